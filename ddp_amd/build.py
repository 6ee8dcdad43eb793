"""Build libddp_mi355x.so in-tree with hipcc for gfx950 (no JIT cache: the .so travels with the tree)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB_DIR = os.path.join(HERE, 'lib')
LIB_PATH = os.path.join(LIB_DIR, 'libddp_mi355x.so')
SOURCES = ['ddp_api.hip', 'ddp_gemm.hip', 'ddp_gemm_bf16.hip', 'ddp_kernels.hip', 'ddp_layer_tail.hip', 'ddp_step_record.hip',
           'ddp_noise.hip', 'ddp_ddpm_chain.hip', 'ddp_hints.hip', 'ddp_prior_start.hip', 'ddp_fcn_gn.hip', 'ddp_class_prior.hip',
           'ddp_score_prior.hip']
HEADERS = ['exports.map', 'ddp_internal.h', 'gemm_f32.h', 'gemm_bf16x3.h', 'layer_bf16x3.h', os.path.join('..', '..', 'include', 'ddp_mi355x.h')]
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-Wall', '-Wno-unused-function']


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return 'hipcc'


def source_hash():
    """sha256 (16 hex digits) over the kernel sources + the C-ABI header: names the code state a profile was taken from
    (profiles/*_pmc_summary.json carry it; bench.py only quotes PMC traffic measured on the SAME sources)."""
    import hashlib
    h = hashlib.sha256()
    for s in sorted(SOURCES + HEADERS):
        with open(os.path.join(CSRC, s), 'rb') as f:
            h.update(s.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


STAMP_PATH = os.path.join(LIB_DIR, '.source_sha')


def built_hash():
    """source_hash() of the sources the .so in lib/ was built from ('' when there is no stamp)."""
    try:
        with open(STAMP_PATH) as f:
            return f.read().strip()
    except OSError:
        return ''


def needs_build():
    # by CONTENT, not by mtime: after a fresh checkout (or a gpurun snapshot) mtimes are arbitrary, and the .so is git-ignored
    return not os.path.exists(LIB_PATH) or built_hash() != source_hash()


# test-only probe of the elementwise __device__ functions (tests/probe/, tests/test_device_math_gpu.py): its own library and its
# own stamp, outside source_hash(); ddp_amd never loads it and libddp_mi355x.so does not contain it
PROBE_SRC = os.path.join(HERE, '..', 'tests', 'probe', 'device_math_probe.hip')
PROBE_LIB_PATH = os.path.join(LIB_DIR, 'libddp_probe.so')
PROBE_STAMP_PATH = os.path.join(LIB_DIR, '.probe_sha')


def probe_hash():
    """sha256 (16 hex digits) over the probe source + the csrc headers it includes"""
    import hashlib
    h = hashlib.sha256()
    for name, path in [('device_math_probe.hip', PROBE_SRC)] + [(s, os.path.join(CSRC, s)) for s in sorted(HEADERS)]:
        with open(path, 'rb') as f:
            h.update(name.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


def probe_built_hash():
    try:
        with open(PROBE_STAMP_PATH) as f:
            return f.read().strip()
    except OSError:
        return ''


def probe_needs_build():
    return not os.path.exists(PROBE_LIB_PATH) or probe_built_hash() != probe_hash()


def probe_cmd(out_path):
    """the one hipcc line of the probe (no object file in between): the product FLAGS + the csrc include path"""
    return [_hipcc()] + FLAGS + ['-I', CSRC, '-x', 'hip', '-shared', os.path.normpath(PROBE_SRC), '-o', out_path]


def _start_probe(force, verbose):
    """start the probe's hipcc (or nothing, when it is current); -> finish(), which waits for it and writes the stamp"""
    if not force and not probe_needs_build():
        return lambda: PROBE_LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    sha = probe_hash()                   # hashed BEFORE compiling, as in build()
    if os.path.exists(PROBE_STAMP_PATH):
        os.remove(PROBE_STAMP_PATH)
    cmd = probe_cmd(PROBE_LIB_PATH)
    if verbose:
        print(' '.join(cmd), flush=True)
    proc = subprocess.Popen(cmd)

    def finish():
        if proc.wait() != 0:
            raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
        with open(PROBE_STAMP_PATH, 'w') as f:
            f.write(sha + '\n')
        return PROBE_LIB_PATH
    return finish


def build_probe(force=False, verbose=True):
    return _start_probe(force, verbose)()


# device-side pre_eval statistics (include/ddp_eval_mi355x.h, ddp_amd/evaluation.py): a library and a stamp of their own, outside
# source_hash() - no part of the sampler ABI, libddp_mi355x.so does not contain it
EVAL_CSRC = os.path.join(CSRC, 'eval')
EVAL_SOURCES = ['ddp_eval.hip']
EVAL_HEADERS = ['eval_exports.map', os.path.join('..', '..', '..', 'include', 'ddp_eval_mi355x.h')]
EVAL_LIB_PATH = os.path.join(LIB_DIR, 'libddp_eval.so')
EVAL_STAMP_PATH = os.path.join(LIB_DIR, '.eval_sha')


def eval_hash():
    """sha256 (16 hex digits) over the evaluation sources, their version script and their C-ABI header"""
    import hashlib
    h = hashlib.sha256()
    for s in sorted(EVAL_SOURCES + EVAL_HEADERS):
        with open(os.path.join(EVAL_CSRC, s), 'rb') as f:
            h.update(s.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


def eval_built_hash():
    try:
        with open(EVAL_STAMP_PATH) as f:
            return f.read().strip()
    except OSError:
        return ''


def eval_needs_build():
    return not os.path.exists(EVAL_LIB_PATH) or eval_built_hash() != eval_hash()


def eval_cmd(out_path):
    """the one hipcc line of the evaluation library (no object file in between): the product FLAGS + its version script"""
    return ([_hipcc()] + FLAGS + ['-x', 'hip', '-shared'] + [os.path.join(EVAL_CSRC, s) for s in EVAL_SOURCES]
            + ['-Wl,--version-script=' + os.path.join(EVAL_CSRC, 'eval_exports.map'), '-o', out_path])


def _start_eval(force, verbose):
    """start the evaluation library's hipcc (or nothing, when it is current); -> finish(), as _start_probe"""
    if not force and not eval_needs_build():
        return lambda: EVAL_LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    sha = eval_hash()                    # hashed BEFORE compiling, as in build()
    if os.path.exists(EVAL_STAMP_PATH):
        os.remove(EVAL_STAMP_PATH)
    cmd = eval_cmd(EVAL_LIB_PATH)
    if verbose:
        print(' '.join(cmd), flush=True)
    proc = subprocess.Popen(cmd)

    def finish():
        if proc.wait() != 0:
            raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
        with open(EVAL_STAMP_PATH, 'w') as f:
            f.write(sha + '\n')
        return EVAL_LIB_PATH
    return finish


def build_eval(force=False, verbose=True):
    return _start_eval(force, verbose)()


# device-side confusion matrix (include/ddp_cm_mi355x.h, ddp_amd/confusion.py): again a library and a stamp of their own, outside
# source_hash() and eval_hash() - neither of the other two libraries contains it
CM_CSRC = os.path.join(CSRC, 'cm')
CM_SOURCES = ['ddp_cm.hip']
CM_HEADERS = ['cm_exports.map', os.path.join('..', '..', '..', 'include', 'ddp_cm_mi355x.h')]
CM_LIB_PATH = os.path.join(LIB_DIR, 'libddp_cm.so')
CM_STAMP_PATH = os.path.join(LIB_DIR, '.cm_sha')


def cm_hash():
    """sha256 (16 hex digits) over the confusion-matrix source, its version script and its C-ABI header"""
    import hashlib
    h = hashlib.sha256()
    for s in sorted(CM_SOURCES + CM_HEADERS):
        with open(os.path.join(CM_CSRC, s), 'rb') as f:
            h.update(s.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


def cm_built_hash():
    try:
        with open(CM_STAMP_PATH) as f:
            return f.read().strip()
    except OSError:
        return ''


def cm_needs_build():
    return not os.path.exists(CM_LIB_PATH) or cm_built_hash() != cm_hash()


def cm_cmd(out_path):
    """the one hipcc line of the confusion-matrix library (no object file in between): the product FLAGS + its version script"""
    return ([_hipcc()] + FLAGS + ['-x', 'hip', '-shared'] + [os.path.join(CM_CSRC, s) for s in CM_SOURCES]
            + ['-Wl,--version-script=' + os.path.join(CM_CSRC, 'cm_exports.map'), '-o', out_path])


def _start_cm(force, verbose):
    """start the confusion-matrix library's hipcc (or nothing, when it is current); -> finish(), as _start_probe"""
    if not force and not cm_needs_build():
        return lambda: CM_LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    sha = cm_hash()                      # hashed BEFORE compiling, as in build()
    if os.path.exists(CM_STAMP_PATH):
        os.remove(CM_STAMP_PATH)
    cmd = cm_cmd(CM_LIB_PATH)
    if verbose:
        print(' '.join(cmd), flush=True)
    proc = subprocess.Popen(cmd)

    def finish():
        if proc.wait() != 0:
            raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
        with open(CM_STAMP_PATH, 'w') as f:
            f.write(sha + '\n')
        return CM_LIB_PATH
    return finish


def build_cm(force=False, verbose=True):
    return _start_cm(force, verbose)()


# device-side LSS lift and pool (include/ddp_lss_mi355x.h, ddp_amd/lss.py): a fourth library with a stamp of its own, outside the
# other three hashes - none of the other libraries contains it
LSS_CSRC = os.path.join(CSRC, 'lss')
LSS_SOURCES = ['ddp_lss.hip']
LSS_HEADERS = ['lss_exports.map', os.path.join('..', '..', '..', 'include', 'ddp_lss_mi355x.h')]
LSS_LIB_PATH = os.path.join(LIB_DIR, 'libddp_lss.so')
LSS_STAMP_PATH = os.path.join(LIB_DIR, '.lss_sha')


def lss_hash():
    """sha256 (16 hex digits) over the LSS source, its version script and its C-ABI header"""
    import hashlib
    h = hashlib.sha256()
    for s in sorted(LSS_SOURCES + LSS_HEADERS):
        with open(os.path.join(LSS_CSRC, s), 'rb') as f:
            h.update(s.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


def lss_built_hash():
    try:
        with open(LSS_STAMP_PATH) as f:
            return f.read().strip()
    except OSError:
        return ''


def lss_needs_build():
    return not os.path.exists(LSS_LIB_PATH) or lss_built_hash() != lss_hash()


def lss_cmd(out_path):
    """the one hipcc line of the LSS library (no object file in between): the product FLAGS + its version script"""
    return ([_hipcc()] + FLAGS + ['-x', 'hip', '-shared'] + [os.path.join(LSS_CSRC, s) for s in LSS_SOURCES]
            + ['-Wl,--version-script=' + os.path.join(LSS_CSRC, 'lss_exports.map'), '-o', out_path])


def _start_lss(force, verbose):
    """start the LSS library's hipcc (or nothing, when it is current); -> finish(), as _start_probe"""
    if not force and not lss_needs_build():
        return lambda: LSS_LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    sha = lss_hash()                     # hashed BEFORE compiling, as in build()
    if os.path.exists(LSS_STAMP_PATH):
        os.remove(LSS_STAMP_PATH)
    cmd = lss_cmd(LSS_LIB_PATH)
    if verbose:
        print(' '.join(cmd), flush=True)
    proc = subprocess.Popen(cmd)

    def finish():
        if proc.wait() != 0:
            raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
        with open(LSS_STAMP_PATH, 'w') as f:
            f.write(sha + '\n')
        return LSS_LIB_PATH
    return finish


def build_lss(force=False, verbose=True):
    return _start_lss(force, verbose)()


# device-side front of DepthLSSTransform (include/ddp_dlss_mi355x.h, ddp_amd/dlss.py): lidar projection, depth scatter and the
# dtransform stem; a fifth library with a stamp of its own, outside the other four hashes - none of the other libraries contains it
DLSS_CSRC = os.path.join(CSRC, 'dlss')
DLSS_SOURCES = ['ddp_dlss.hip']
DLSS_HEADERS = ['dlss_exports.map', os.path.join('..', '..', '..', 'include', 'ddp_dlss_mi355x.h')]
DLSS_LIB_PATH = os.path.join(LIB_DIR, 'libddp_dlss.so')
DLSS_STAMP_PATH = os.path.join(LIB_DIR, '.dlss_sha')


def dlss_hash():
    """sha256 (16 hex digits) over the depth-LSS source, its version script and its C-ABI header"""
    import hashlib
    h = hashlib.sha256()
    for s in sorted(DLSS_SOURCES + DLSS_HEADERS):
        with open(os.path.join(DLSS_CSRC, s), 'rb') as f:
            h.update(s.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


def dlss_built_hash():
    try:
        with open(DLSS_STAMP_PATH) as f:
            return f.read().strip()
    except OSError:
        return ''


def dlss_needs_build():
    return not os.path.exists(DLSS_LIB_PATH) or dlss_built_hash() != dlss_hash()


def dlss_cmd(out_path):
    """the one hipcc line of the depth-LSS library (no object file in between): the product FLAGS + its version script"""
    return ([_hipcc()] + FLAGS + ['-x', 'hip', '-shared'] + [os.path.join(DLSS_CSRC, s) for s in DLSS_SOURCES]
            + ['-Wl,--version-script=' + os.path.join(DLSS_CSRC, 'dlss_exports.map'), '-o', out_path])


def _start_dlss(force, verbose):
    """start the depth-LSS library's hipcc (or nothing, when it is current); -> finish(), as _start_probe"""
    if not force and not dlss_needs_build():
        return lambda: DLSS_LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    sha = dlss_hash()                    # hashed BEFORE compiling, as in build()
    if os.path.exists(DLSS_STAMP_PATH):
        os.remove(DLSS_STAMP_PATH)
    cmd = dlss_cmd(DLSS_LIB_PATH)
    if verbose:
        print(' '.join(cmd), flush=True)
    proc = subprocess.Popen(cmd)

    def finish():
        if proc.wait() != 0:
            raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
        with open(DLSS_STAMP_PATH, 'w') as f:
            f.write(sha + '\n')
        return DLSS_LIB_PATH
    return finish


def build_dlss(force=False, verbose=True):
    return _start_dlss(force, verbose)()


def build(force=False, verbose=True):
    # the probe, the evaluation, confusion-matrix, LSS and depth-LSS libraries compile beside the product's objects; the probe's
    # compile-time checks of the schedule tables make build() fail
    finish_side = [_start_probe(force, verbose), _start_eval(force, verbose), _start_cm(force, verbose), _start_lss(force, verbose),
                   _start_dlss(force, verbose)]
    try:
        path = _build_product(force, verbose)
    except BaseException:
        for finish in finish_side:
            try:
                finish()
            except RuntimeError:
                pass
        raise
    for finish in finish_side:
        finish()
    return path


def _build_product(force, verbose):
    if not force and not needs_build():
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    sha = source_hash()                  # hashed BEFORE compiling: an edit during the build leaves a stale stamp, i.e. a rebuild
    if os.path.exists(STAMP_PATH):
        os.remove(STAMP_PATH)
    objs = []
    procs = []
    for s in SOURCES:
        obj = os.path.join(LIB_DIR, s.replace('.hip', '.o'))
        cmd = [_hipcc()] + FLAGS + ['-x', 'hip', '-c', os.path.join(CSRC, s), '-o', obj]
        if verbose:
            print(' '.join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
    cmd = [_hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,--version-script=' + os.path.join(CSRC, 'exports.map'),
           '-o', LIB_PATH] + objs
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(STAMP_PATH, 'w') as f:
        f.write(sha + '\n')
    return LIB_PATH


if __name__ == '__main__':
    build(force='--force' in sys.argv)
    print(LIB_PATH)
