"""What holds for every library ``ddp_amd/build.py`` describes, asserted once: each side library of ``build.SIDE`` builds, exports
exactly what its header declares, its binding lists and its version script pins, and nothing of another library; it has a stamp, a
hipcc line and a set of hashed files of its own; an edit of one of its files changes its hash and no other.  The product library and
the probe take part wherever the statement is about all libraries.  What is one library's own - struct sizes, the header's
``#define``s, its refusals - is in that library's host file.  No GPU compute is invoked."""
import hashlib
import importlib.util
import itertools
import os
import re
import shutil
import subprocess

import pytest

from ddp_amd import _cm_lib, _dlss_lib, _eval_lib, _lib, _lss_lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINDINGS = {'eval': _eval_lib, 'cm': _cm_lib, 'lss': _lss_lib, 'dlss': _dlss_lib}
NAMES = list(BINDINGS)
# the number of ddp_ symbols each library exports and the ABI version it reports
PRODUCT_EXPORTS, PRODUCT_ABI = 36, 7
SIDE_EXPORTS = {'eval': 6, 'cm': 4, 'lss': 7, 'dlss': 8}
SIDE_ABI = {'eval': 1, 'cm': 1, 'lss': 1, 'dlss': 1}
# the hash of every library's sources.  Whoever edits a kernel source, a header or a version script updates the literal of that
# library; a change that is meant to compile nothing differently (of build.py, of a binding) must leave all six as they are
PINNED = {'source': 'b0afb94619b83ea1', 'probe': '375ba29834b1b527', 'eval': '2f09f27ee8fff064', 'cm': '5bf57f3d5d8adf9e',
          'lss': '07399ef3580a9383', 'dlss': 'cc185233e0601c5a'}


def test_the_table_is_the_four_bindings_in_order():
    assert list(build.SIDE) == NAMES == list(SIDE_EXPORTS) == list(SIDE_ABI)
    assert all(build.SIDE[n].name == n for n in NAMES)
    assert all(b._binding.side is build.SIDE[n] and b._binding.abi_version == b.ABI_VERSION for n, b in BINDINGS.items())


def _sha(names, base):
    """the hash rule restated without a call of build.py"""
    h = hashlib.sha256()
    for s in sorted(names):
        with open(os.path.join(base, s), 'rb') as f:
            h.update(s.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


def _all_hashes(b):
    return dict(source=b.source_hash(), probe=b.probe_hash(), **{n: b.SIDE[n].hash() for n in b.SIDE})


def _dyn_syms(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if ' T ' in l)


def _foreign(syms, own):
    """the symbols that carry the prefix of a side library other than ``own``"""
    return [s for s in syms for n in NAMES if n != own and s.startswith('ddp_' + n)]


# ---- 1, 2: it builds and exports exactly the header ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_library_builds_and_exports_exactly_the_header(name):
    side, M = build.SIDE[name], BINDINGS[name]
    path = side.start(verbose=False)()
    assert path == side.lib_path and os.path.exists(path) and not side.needs_build() and side.built_hash() == side.hash()
    header = open(os.path.join(ROOT, 'include', f'ddp_{name}_mi355x.h')).read()
    declared = sorted(set(re.findall(rf'\b(ddp_{name}_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S))))
    syms = _dyn_syms(path)
    assert syms == declared == sorted(M.EXPORTS) and len(declared) == SIDE_EXPORTS[name]
    script = open(os.path.join(side.csrc, f'{name}_exports.map')).read()
    assert sorted(re.findall(rf'\b(ddp_{name}_\w+);', script)) == declared and 'local:\n    *;' in script
    assert not _foreign(syms, name) and all(s.startswith(f'ddp_{name}_') for s in syms)
    lib = M.load()
    assert getattr(lib, f'ddp_{name}_abi_version')() == SIDE_ABI[name] == M.ABI_VERSION
    assert f'#define DDP_{name.upper()}_ABI_VERSION {SIDE_ABI[name]}' in header


def test_product_library_exports_nothing_of_a_side_library():
    build.build(verbose=False)
    assert not build.needs_build() and build.built_hash() == build.source_hash()
    syms = [s for s in _dyn_syms(_lib.lib_path()) if 'ddp_' in s]
    assert syms == sorted(_lib.EXPORTS) and len(syms) == PRODUCT_EXPORTS and not _foreign(syms, None)
    assert _lib.ABI_VERSION == PRODUCT_ABI == _lib.load().ddp_abi_version()
    # and after the whole build every side library is what the test above saw
    for name in NAMES:
        syms = _dyn_syms(build.SIDE[name].lib_path)
        assert syms == sorted(BINDINGS[name].EXPORTS) and len(syms) == SIDE_EXPORTS[name] and not _foreign(syms, name)
        assert not set(syms) & set(_lib.EXPORTS)


# ---- 3, 4: paths and the command line --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_paths_and_command_are_its_own(name):
    side = build.SIDE[name]
    assert side.stamp_path.endswith(os.path.join('lib', f'.{name}_sha')) and side.lib_path.endswith(os.path.join('lib', f'libddp_{name}.so'))
    assert os.path.dirname(side.stamp_path) == os.path.dirname(side.lib_path) == build.LIB_DIR
    cmd = side.cmd('x.so')
    assert cmd[1:1 + len(build.FLAGS)] == build.FLAGS and cmd[-2:] == ['-o', 'x.so'] and '-c' not in cmd
    assert [a for a in cmd if a.endswith('.hip')] == [os.path.join(side.csrc, f'ddp_{name}.hip')] and side.sources == [f'ddp_{name}.hip']
    assert [a for a in cmd if a.startswith('-Wl,--version-script=')] == ['-Wl,--version-script=' + os.path.join(side.csrc, f'{name}_exports.map')]


def test_stamps_and_libraries_are_pairwise_distinct():
    libs = [build.PROBE, *build.SIDE.values()]
    assert len({build.STAMP_PATH, *(l.stamp_path for l in libs)}) == 2 + len(NAMES) == 6
    assert len({build.LIB_PATH, *(l.lib_path for l in libs)}) == 6
    assert build.PROBE.stamp_path.endswith(os.path.join('lib', '.probe_sha')) and build.PROBE_LIB_PATH == build.PROBE.lib_path


# ---- 5, 6, 8: what is hashed -------------------------------------------------------------------------------------------------------------
def _hashed_files():
    sets = {'source': {os.path.normpath(os.path.join(build.CSRC, s)) for s in build.SOURCES + build.HEADERS}}
    for name, side in build.SIDE.items():
        sets[name] = {os.path.normpath(os.path.join(side.csrc, s)) for s in side.sources + side.headers}
    return sets


def test_hashed_file_sets_are_pairwise_disjoint():
    sets = _hashed_files()
    assert all(os.path.exists(p) for s in sets.values() for p in s)
    for a, b in itertools.combinations(sets, 2):
        assert not sets[a] & sets[b], (a, b)
    for name in NAMES:
        assert os.path.normpath(os.path.join(ROOT, 'include', f'ddp_{name}_mi355x.h')) in sets[name] and len(sets[name]) == 3
    assert os.path.normpath(os.path.join(ROOT, 'include', 'ddp_mi355x.h')) in sets['source']


def test_hashes_are_distinct_and_equal_the_restated_rule():
    got = _all_hashes(build)
    assert list(got) == ['source', 'probe'] + NAMES and len(set(got.values())) == 6
    assert got['source'] == _sha(build.SOURCES + build.HEADERS, build.CSRC)
    for name, side in build.SIDE.items():
        assert got[name] == _sha(side.sources + side.headers, side.csrc) == side.hash()
    assert all(re.fullmatch(r'[0-9a-f]{16}', v) for v in got.values())


def test_hashes_are_the_pinned_ones():
    assert _all_hashes(build) == PINNED


# ---- 7: an edit of one library's file is that library's alone ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_an_edit_changes_its_hash_and_no_other(name, tmp_path):
    for d in ('ddp_amd', 'include', os.path.join('tests', 'probe')):
        shutil.copytree(os.path.join(ROOT, d), tmp_path / d, ignore=shutil.ignore_patterns('lib', 'lib_*', '__pycache__'))
    spec = importlib.util.spec_from_file_location('_build_of_the_copy_' + name, str(tmp_path / 'ddp_amd' / 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)                           # build.py finds its sources beside itself
    side = b.SIDE[name]
    assert side.csrc.startswith(str(tmp_path)) and side.lib_path.startswith(str(tmp_path))
    before = first = _all_hashes(b)
    assert before == _all_hashes(build)
    files = sorted(_hashed_files()[name])
    assert len(files) == 3
    for path in files:                                   # the source, the version script, the header
        with open(os.path.join(str(tmp_path), os.path.relpath(path, ROOT)), 'a') as f:
            f.write('\n')
        after = _all_hashes(b)
        assert after[name] != before[name] and side.needs_build()
        assert {k: v for k, v in after.items() if k != name} == {k: v for k, v in before.items() if k != name}
        before = after
    assert _all_hashes(build) == first                   # the tree itself was not touched
