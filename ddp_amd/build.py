"""Build libddp_mi355x.so and the libraries beside it in-tree with hipcc for gfx950 (no JIT cache: the .so files travel with the tree).

The product library is compiled per object and linked (``_build_product``).  Every other library is ONE hipcc line, described by a
``Lib``: the test-only ``PROBE`` and the table ``SIDE`` of the device features that are no part of the sampler ABI.  Adding a side
library is a directory ``csrc/<name>/`` with its sources and ``<name>_exports.map``, a header ``include/ddp_<name>_mi355x.h``, one
``Side`` row, and a binding file on ``_sidelib``.  The row goes into ``LATER``: ``SIDE`` is the table of four that
tests/test_build_host.py pins by name and hash, and stays as it is.
"""
import hashlib
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
STAMP_PATH = os.path.join(LIB_DIR, '.source_sha')


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return 'hipcc'


def _sha(base, names, first=()):
    """sha256 (16 hex digits) over name + NUL + content of the files: the (name, path) pairs ``first``, then the SORTED ``names`` of
    directory ``base``"""
    h = hashlib.sha256()
    for s, path in list(first) + [(s, os.path.join(base, s)) for s in sorted(names)]:
        with open(path, 'rb') as f:
            h.update(s.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


def _stamp(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return ''


def source_hash():
    """sha256 (16 hex digits) over the kernel sources + the C-ABI header: names the code state a profile was taken from
    (profiles/*_pmc_summary.json carry it; bench.py only quotes PMC traffic measured on the SAME sources)."""
    return _sha(CSRC, SOURCES + HEADERS)


def built_hash():
    """source_hash() of the sources the .so in lib/ was built from ('' when there is no stamp)."""
    return _stamp(STAMP_PATH)


def needs_build():
    # by CONTENT, not by mtime: after a fresh checkout (or a gpurun snapshot) mtimes are arbitrary, and the .so is git-ignored
    return not os.path.exists(LIB_PATH) or built_hash() != source_hash()


class Lib:
    """A library beside the product's, built by one hipcc line (no object file in between), with a stamp of its own,
    ``lib/.<name>_sha``, outside source_hash() and every other library's hash: no library contains another.  What is hashed and what
    the hipcc line holds, ``hash()`` and ``cmd(out_path)``, is the subclass's."""

    def __init__(self, name):
        self.name = name
        self.lib_path = os.path.join(LIB_DIR, f'libddp_{name}.so')
        self.stamp_path = os.path.join(LIB_DIR, f'.{name}_sha')

    def built_hash(self):
        """hash() of the sources the .so in lib/ was built from ('' when there is no stamp)"""
        return _stamp(self.stamp_path)

    def needs_build(self):
        return not os.path.exists(self.lib_path) or self.built_hash() != self.hash()

    def start(self, force=False, verbose=True):
        """start the hipcc (or nothing, when the library is current); -> finish(), which waits for it and writes the stamp"""
        if not force and not self.needs_build():
            return lambda: self.lib_path
        os.makedirs(LIB_DIR, exist_ok=True)
        sha = self.hash()                # hashed BEFORE compiling: an edit during the build leaves a stale stamp, i.e. a rebuild
        if os.path.exists(self.stamp_path):
            os.remove(self.stamp_path)
        cmd = self.cmd(self.lib_path)
        if verbose:
            print(' '.join(cmd), flush=True)
        proc = subprocess.Popen(cmd)

        def finish():
            if proc.wait() != 0:
                raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
            with open(self.stamp_path, 'w') as f:
                f.write(sha + '\n')
            return self.lib_path
        return finish


class Side(Lib):
    """A device feature with a C ABI of its own: ``csrc/<name>/`` holds ``sources`` and the version script ``<name>_exports.map``;
    the script and ``include/ddp_<name>_mi355x.h`` are hashed with the sources."""

    def __init__(self, name, sources):
        super().__init__(name)
        self.csrc = os.path.join(CSRC, name)
        self.sources = sources
        self.headers = [name + '_exports.map', os.path.join('..', '..', '..', 'include', f'ddp_{name}_mi355x.h')]

    def hash(self):
        """sha256 (16 hex digits) over the sources, the version script and the C-ABI header"""
        return _sha(self.csrc, self.sources + self.headers)

    def cmd(self, out_path):
        """the hipcc line: the product FLAGS + the library's version script"""
        return ([_hipcc()] + FLAGS + ['-x', 'hip', '-shared'] + [os.path.join(self.csrc, s) for s in self.sources]
                + ['-Wl,--version-script=' + os.path.join(self.csrc, self.headers[0]), '-o', out_path])


# test-only probe of the elementwise __device__ functions (tests/probe/, tests/test_device_math_gpu.py): ddp_amd never loads it and
# libddp_mi355x.so does not contain it.  It lives outside csrc/ and has no version script: its source + the csrc headers it includes
# are what is hashed, and the csrc include path is what its hipcc line adds
PROBE_SRC = os.path.join(HERE, '..', 'tests', 'probe', 'device_math_probe.hip')


class _Probe(Lib):
    def hash(self):
        return _sha(CSRC, HEADERS, first=[('device_math_probe.hip', PROBE_SRC)])

    def cmd(self, out_path):
        return [_hipcc()] + FLAGS + ['-I', CSRC, '-x', 'hip', '-shared', os.path.normpath(PROBE_SRC), '-o', out_path]


PROBE = _Probe('probe')
PROBE_LIB_PATH = PROBE.lib_path
probe_hash, probe_built_hash, probe_cmd = PROBE.hash, PROBE.built_hash, PROBE.cmd

# pre_eval statistics (ddp_amd/evaluation.py), confusion matrix (confusion.py), LSS lift and pool (lss.py), and the front of
# DepthLSSTransform - lidar projection, depth scatter, dtransform stem (dlss.py)
SIDE = {lib.name: lib for lib in (Side('eval', ['ddp_eval.hip']), Side('cm', ['ddp_cm.hip']), Side('lss', ['ddp_lss.hip']),
                                  Side('dlss', ['ddp_dlss.hip']))}

# side libraries added after the table of four was pinned by tests/test_build_host.py: hard voxelisation of lidar points (vox.py)
LATER = {lib.name: lib for lib in (Side('vox', ['ddp_vox.hip']),)}


def build(force=False, verbose=True):
    # the probe and the side libraries compile beside the product's objects; the probe's compile-time checks of the schedule tables
    # make build() fail
    finish_side = [lib.start(force, verbose) for lib in [PROBE, *SIDE.values(), *LATER.values()]]
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
