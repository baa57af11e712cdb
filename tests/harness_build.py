"""What the tests/*_harness.py modules share: a temporary directory per harness (removed at exit), the one set of compile flags, g++
into a shared library that is loaded, g++ into the stand-alone program of the same source, and an array's ``void*``."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

CXXFLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
_dirs = {}


def tmp(name):
    if name not in _dirs:
        _dirs[name] = tempfile.mkdtemp(prefix=name + "_harness_")
        atexit.register(shutil.rmtree, _dirs[name], ignore_errors=True)
    return _dirs[name]


def load_library(name, src):
    """`src` compiled into ``lib<name>.so`` in tmp(name), loaded"""
    so = os.path.join(tmp(name), f"lib{name}.so")
    subprocess.check_call(["g++"] + CXXFLAGS + ["-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def build_program(name, src, define, extra_flags=()):
    """`src` compiled with -D`define` (and `extra_flags`) into a program in tmp(name); returns (program, path for its case file)"""
    exe, data = os.path.join(tmp(name), name + "_standalone"), os.path.join(tmp(name), "cases.bin")
    subprocess.check_call(["g++"] + CXXFLAGS + list(extra_flags) + ["-D" + define, "-o", exe, src])
    return exe, data


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)
