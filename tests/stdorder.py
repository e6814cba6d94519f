"""Loader of tests/_stdorder.cpp: compiled with the system C++ compiler into a directory the caller gives (a tmp_path)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class StdOrder:
    def __init__(self, outdir):
        so = os.path.join(str(outdir), "libstdorder.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(_HERE, "_stdorder.cpp")])
        self._L = C.CDLL(so)
        self._L.std_shuffle.argtypes = [C.c_int64, C.c_void_p]
        self._L.std_sort_by_key.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]

    def shuffle(self, items):
        """std::shuffle(items, std::default_random_engine(0))."""
        perm = np.zeros(len(items), np.int64)
        if len(items):
            self._L.std_shuffle(len(items), perm.ctypes.data)
        return [items[i] for i in perm]

    def sort(self, items, key):
        """std::sort(items) with operator< comparing key(item) (not stable: the library's own order among equal keys)."""
        keys = np.ascontiguousarray([key(x) for x in items], np.int64)
        perm = np.arange(len(items), dtype=np.int64)
        if len(items):
            self._L.std_sort_by_key(len(items), keys.ctypes.data, perm.ctypes.data)
        return [items[i] for i in perm]
