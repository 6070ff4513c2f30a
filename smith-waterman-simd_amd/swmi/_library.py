"""The one loader of the satellite libraries that link libswmi.so: swmi.wide, swmi.wide_long,
swmi.wide_profile and the four banded modules each hold a Library, or a binding body that is one."""
import ctypes
import os

from . import ERR_NOT_INITIALIZED, SwmiError
from . import load as _load_swmi

_HERE = os.path.dirname(os.path.abspath(__file__))


class Library:
    """One library: its entries are `prefix`_<name>.  The file is `lib_file` beside libswmi.so, or what the variable `env` names
    at import; `declare(lib)` sets the argtypes and restypes on the freshly opened CDLL (last_error's is set here)."""

    def __init__(self, prefix, lib_file, env, declare):
        self.prefix, self._declare = prefix, declare
        self.lib_path = os.environ.get(env, os.path.join(os.path.dirname(_HERE), "lib", lib_file))
        self._lib, self._entries = None, {}

    def load(self):
        if self._lib is not None:
            return self._lib
        _load_swmi()            # libswmi.so, which the library links
        if not os.path.exists(self.lib_path):
            raise SwmiError(ERR_NOT_INITIALIZED,
                            "%s not built: run __graft_entry__.build() or make -C smith-waterman-simd_amd/csrc" % self.lib_path)
        lib = ctypes.CDLL(self.lib_path)
        getattr(lib, self.prefix + "_last_error").restype = ctypes.c_char_p
        self._declare(lib)
        self._lib = lib
        return lib

    def entry(self, name):
        """`prefix`_<name> of the loaded library, bound once: the smallest calls are short enough for the lookup to show."""
        entry = self._entries.get(name)
        if entry is None:
            entry = self._entries[name] = getattr(self.load(), self.prefix + "_" + name)
        return entry

    def last_error(self):
        return self.entry("last_error")().decode()

    def version(self):
        return int(self.entry("version")())

    def check(self, rc):
        if rc < 0:
            raise SwmiError(rc, self.last_error())
        return rc
