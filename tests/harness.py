"""The one loader of the C++/HIP test artefacts under tests/cpp (built by tests/cpp/Makefile, one target per artefact).

An artefact that is missing, or older than one of its own sources, is rebuilt by name before it is handed out.  Its own sources are the
.cpp / .hip files it is made of, never headers: built artefacts travel to the GPU box, and a header's timestamp there must not start a
compile in the middle of a test run."""
import ctypes
import os
import subprocess

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
# what an artefact is made of besides the source that carries its name
ALSO = {"libshimtest.so": ["arguments_test.cpp"], "libarithdev_pasta.so": ["arithdev.hip"], "entries_latency_test": ["entriestest.hip"]}


def path(name):
    return os.path.join(CPP, name)


def sources(name):
    """libXtest.so <- X_test.cpp, libX.so <- X.hip, program X <- X.hip (the library names drop the underscores of X), plus ALSO."""
    stem = name[3:-3] if name.endswith(".so") else name
    own = [f for f in sorted(os.listdir(CPP)) if f.endswith((".cpp", ".hip")) and f[:-4].replace("_", "") == stem.replace("_", "")]
    assert len(own) == 1, "tests/cpp: %s has no source of its name (%r)" % (name, own)
    return [path(f) for f in own + ALSO.get(name, [])]


def stale(artefact, srcs):
    return not os.path.exists(artefact) or os.path.getmtime(artefact) < max(os.path.getmtime(s) for s in srcs)


def _fresh(name):
    if stale(path(name), sources(name)):
        subprocess.check_call(["make", "-C", CPP, name])
    return path(name)


def library(name):
    return ctypes.CDLL(_fresh(name))


def program(name):
    return _fresh(name)
