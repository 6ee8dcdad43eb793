"""What the ctypes bindings of the side libraries (``build.SIDE``: ``_eval_lib``, ``_cm_lib``, ``_lss_lib``, ``_dlss_lib``;
``build.LATER``: ``_vox_lib``) share:
load once per path, refuse a missing, stale or other-ABI library, turn a return code into an exception.

Like ``_lib``: NO fallback.  A missing or stale library raises; build it with ``python -m ddp_amd.build``.  A binding file holds
what is the library's own - constants, structs, ``EXPORTS``, the argument types, its error class - and one ``Binding``.
"""
import ctypes as C
import os


class SideLibError(RuntimeError):
    """base of DdpEvalError, DdpCmError, DdpLssError, DdpDlssError, DdpVoxError: ``code`` is the library's return code (None: raised on loading)"""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class Binding:
    """``side``: the library's ``build.SIDE`` or ``build.LATER`` entry, which names it (libddp_<name>.so, symbols ddp_<name>_*); ``argtypes``: {symbol:
    argument types} of its entry points, which all return an int code, beside ``ddp_<name>_last_error`` and ``ddp_<name>_abi_version``;
    ``module``: the public module the messages name; ``error``: the binding's SideLibError; ``badcfg``: the return code that means a
    refused configuration and raises ValueError (None: ``error``, like every other code)."""

    def __init__(self, side, abi_version, argtypes, module, error, badcfg=None):
        self.side, self.abi_version, self.argtypes, self.module, self.error, self.badcfg = side, abi_version, argtypes, module, error, badcfg
        self.prefix = f'ddp_{side.name}_'
        self.libs = {}

    def load(self, path=None):
        """Load (once per path) and return the library; raises when it is missing or was built from other sources."""
        side = self.side
        path = os.path.abspath(path or side.lib_path)
        if path in self.libs:
            return self.libs[path]
        if not os.path.exists(path):
            raise self.error(f'{path} not found: build it with `python -m ddp_amd.build` (hipcc --offload-arch=gfx950); '
                             f'{self.module} has no non-HIP fallback')
        # the in-tree library is git-ignored: a checkout / snapshot may carry one built from OTHER sources
        if path == os.path.abspath(side.lib_path) and side.built_hash() != side.hash():
            raise self.error(f'{path} is stale: built from sources {side.built_hash() or "<no stamp>"}, the tree holds '
                             f'{side.hash()}; rebuild with `python -m ddp_amd.build`')
        lib = C.CDLL(path)
        last_error, abi_version = getattr(lib, self.prefix + 'last_error'), getattr(lib, self.prefix + 'abi_version')
        last_error.restype, last_error.argtypes = C.c_char_p, []
        abi_version.restype, abi_version.argtypes = C.c_int, []
        for name, argtypes in self.argtypes.items():
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = argtypes
        if abi_version() != self.abi_version:
            raise self.error(f'ABI mismatch: library {abi_version()} vs binding {self.abi_version}')
        self.libs[path] = lib
        return lib

    def check(self, rc, lib=None):
        if rc != 0:
            msg = getattr(lib or self.load(), self.prefix + 'last_error')().decode()
            if rc == self.badcfg:
                raise ValueError(f'libddp_{self.side.name} refused the configuration: {msg}')
            raise self.error(f'libddp_{self.side.name} error {rc}: {msg}', rc)
