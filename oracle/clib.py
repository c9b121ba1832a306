"""ORACLE (test infrastructure): ctypes loader of oracle/liboracle.so (gcc build of oracle/*.c).

The library is rebuilt when it is absent or older than one of its sources (the Makefile included), so that a library left over
from before a source changed is never loaded; and every `oracle_*` function the sources define must be found in what was loaded
-- a library that lacks one is reported by name here, not by an AttributeError at the first call."""
import ctypes as C
import glob
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_HERE, "liboracle.so")
_EXPORT = re.compile(r"^[A-Za-z_][A-Za-z_0-9]*\s*\**\s*(oracle_[A-Za-z_0-9]+)\(", re.M)


def sources():
    return sorted(glob.glob(os.path.join(_HERE, "*.c"))) + [os.path.join(_HERE, "Makefile")]


def stale():
    """the library is absent, or a source is newer than it"""
    if not os.path.exists(_PATH):
        return True
    built = os.path.getmtime(_PATH)
    return any(os.path.getmtime(s) > built for s in sources())


def exported():
    """the names of the `oracle_*` functions the C sources define"""
    names = set()
    for s in sources()[:-1]:
        with open(s) as f:
            names.update(_EXPORT.findall(f.read()))
    return sorted(names)


def build():
    try:
        subprocess.check_call(["make", "-s", "-C", _HERE])
    except (OSError, subprocess.CalledProcessError) as e:
        raise RuntimeError(f"oracle: `make -C {_HERE}` failed ({e}); {_PATH} is absent or older than its sources and cannot be used") from e


def load():
    if stale():
        build()
    lib = C.CDLL(_PATH)
    missing = [n for n in exported() if not hasattr(lib, n)]
    if missing:
        raise RuntimeError(f"oracle: {_PATH} lacks {', '.join(missing)}: it was built from other sources than oracle/*.c -- "
                           f"remove it (or run `make -C {_HERE} clean`) and import again")
    return lib


lib = load()
