"""The per-library statements of tests/test_build_host.py restated for ``build.LATER``, the table of the side libraries added after
``build.SIDE`` was pinned there: each builds, exports exactly what its header declares, its binding lists and its version script
pins, and nothing of another library; it has a stamp, a hipcc line and three hashed files of its own; an edit of one of its files
changes its hash and none of the six pinned ones; its hash literal is pinned here; ``build.SIDE`` is still the four.  No GPU compute
is invoked."""
import importlib.util
import itertools
import os
import re
import shutil

import pytest

from ddp_amd import _lib, _vox_lib, build
from support import dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINDINGS = {'vox': _vox_lib}
NAMES = list(BINDINGS)
LATER_EXPORTS = {'vox': 9}
LATER_ABI = {'vox': 1}
# whoever edits a source, the header or the version script of a library updates its literal
PINNED = {'vox': '67e1538138b5f999'}
EARLIER = ['source', 'probe', 'eval', 'cm', 'lss', 'dlss']


def _earlier_hashes(b):
    return dict(source=b.source_hash(), probe=b.probe_hash(), **{n: b.SIDE[n].hash() for n in b.SIDE})


def _hashed(side):
    return {os.path.normpath(os.path.join(side.csrc, s)) for s in side.sources + side.headers}


def test_the_tables():
    assert list(build.SIDE) == ['eval', 'cm', 'lss', 'dlss'] and list(build.LATER) == NAMES == list(LATER_EXPORTS) == list(LATER_ABI)
    assert not set(build.SIDE) & set(build.LATER) and list(_earlier_hashes(build)) == EARLIER
    for n, b in BINDINGS.items():
        side = build.LATER[n]
        assert type(side) is build.Side and side.name == n and b._binding.side is side and b._binding.abi_version == b.ABI_VERSION


@pytest.mark.parametrize('name', NAMES)
def test_library_builds_and_exports_exactly_the_header(name):
    side, M = build.LATER[name], BINDINGS[name]
    path = side.start(verbose=False)()
    assert path == side.lib_path and os.path.exists(path) and not side.needs_build() and side.built_hash() == side.hash()
    header = open(os.path.join(ROOT, 'include', f'ddp_{name}_mi355x.h')).read()
    declared = sorted(set(re.findall(rf'\b(ddp_{name}_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S))))
    syms = [s for s in dynamic_symbols(path) if 'ddp_' in s]
    assert syms == declared == sorted(M.EXPORTS) and len(declared) == LATER_EXPORTS[name]
    script = open(os.path.join(side.csrc, f'{name}_exports.map')).read()
    assert sorted(re.findall(rf'\b(ddp_{name}_\w+);', script)) == declared and 'local:\n    *;' in script
    others = [n for n in (*build.SIDE, *build.LATER) if n != name]
    assert all(s.startswith(f'ddp_{name}_') for s in syms) and not [s for s in syms for n in others if s.startswith('ddp_' + n)]
    assert not set(syms) & set(_lib.EXPORTS)
    lib = M.load()
    assert getattr(lib, f'ddp_{name}_abi_version')() == LATER_ABI[name] == M.ABI_VERSION
    assert f'#define DDP_{name.upper()}_ABI_VERSION {LATER_ABI[name]}' in header


def test_the_whole_build_makes_it_too(monkeypatch):
    started = []
    for lib in (build.PROBE, *build.SIDE.values(), *build.LATER.values()):
        monkeypatch.setattr(lib, 'start', lambda force=False, verbose=True, lib=lib: started.append(lib.name) or (lambda: lib.lib_path))
    monkeypatch.setattr(build, '_build_product', lambda force, verbose: build.LIB_PATH)
    assert build.build(verbose=False) == build.LIB_PATH and started == ['probe', 'eval', 'cm', 'lss', 'dlss', *NAMES]


@pytest.mark.parametrize('name', NAMES)
def test_paths_command_and_files_are_its_own(name):
    side = build.LATER[name]
    assert side.stamp_path.endswith(os.path.join('lib', f'.{name}_sha')) and side.lib_path.endswith(os.path.join('lib', f'libddp_{name}.so'))
    assert os.path.dirname(side.stamp_path) == os.path.dirname(side.lib_path) == build.LIB_DIR
    earlier = [build.PROBE, *build.SIDE.values()]
    assert side.stamp_path not in {build.STAMP_PATH, *(l.stamp_path for l in earlier)}
    assert side.lib_path not in {build.LIB_PATH, *(l.lib_path for l in earlier)}
    cmd = side.cmd('x.so')
    assert cmd[1:1 + len(build.FLAGS)] == build.FLAGS and cmd[-2:] == ['-o', 'x.so'] and '-c' not in cmd
    assert [a for a in cmd if a.endswith('.hip')] == [os.path.join(side.csrc, f'ddp_{name}.hip')] and side.sources == [f'ddp_{name}.hip']
    assert [a for a in cmd if a.startswith('-Wl,--version-script=')] == ['-Wl,--version-script=' + os.path.join(side.csrc, f'{name}_exports.map')]
    # its three hashed files: the source, the version script, the header - disjoint from every other library's
    mine = _hashed(side)
    assert len(mine) == 3 and all(os.path.exists(p) for p in mine)
    assert os.path.normpath(os.path.join(ROOT, 'include', f'ddp_{name}_mi355x.h')) in mine
    sets = {'source': {os.path.normpath(os.path.join(build.CSRC, s)) for s in build.SOURCES + build.HEADERS},
            'probe': {os.path.normpath(build.PROBE_SRC)}, **{n: _hashed(s) for n, s in (*build.SIDE.items(), *build.LATER.items())}}
    for a, b in itertools.combinations(sets, 2):
        if name in (a, b):
            assert not sets[a] & sets[b], (a, b)


@pytest.mark.parametrize('name', NAMES)
def test_hash_is_pinned_and_distinct(name):
    got = build.LATER[name].hash()
    assert re.fullmatch(r'[0-9a-f]{16}', got) and got not in _earlier_hashes(build).values()
    assert got == PINNED[name]


@pytest.mark.parametrize('name', NAMES)
def test_an_edit_changes_its_hash_and_none_of_the_six(name, tmp_path):
    for d in ('ddp_amd', 'include', os.path.join('tests', 'probe')):
        shutil.copytree(os.path.join(ROOT, d), tmp_path / d, ignore=shutil.ignore_patterns('lib', 'lib_*', '__pycache__'))
    spec = importlib.util.spec_from_file_location('_build_of_the_copy_later_' + name, str(tmp_path / 'ddp_amd' / 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)                           # build.py finds its sources beside itself
    side = b.LATER[name]
    assert side.csrc.startswith(str(tmp_path)) and side.lib_path.startswith(str(tmp_path))
    six, before = _earlier_hashes(b), side.hash()
    assert six == _earlier_hashes(build) and before == build.LATER[name].hash()
    others = {n: s.hash() for n, s in b.LATER.items() if n != name}
    for path in sorted(_hashed(build.LATER[name])):      # the source, the version script, the header
        with open(os.path.join(str(tmp_path), os.path.relpath(path, ROOT)), 'a') as f:
            f.write('\n')
        after = side.hash()
        assert after != before and side.needs_build()
        assert _earlier_hashes(b) == six and {n: s.hash() for n, s in b.LATER.items() if n != name} == others
        before = after
    assert build.LATER[name].hash() == PINNED[name]      # the tree itself was not touched
