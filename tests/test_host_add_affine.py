"""xyzz_add_affine (curve.hpp: the first real addition of a bucket, affine + affine) against xyzz_madd(from_affine(a), b) on the host build
of the group law: tests/cpp/add_affine_test.cpp, a program that stands alone -- per coordinate field of BLS12-381, BN254, Pallas and Vesta,
1 000 random pairs and the edge cases listed at its top, X / Y / ZZ / ZZZ compared after canonicalisation.  Once as built, once under
AddressSanitizer + UBSan (the program links its own sanitizer runtime; nothing is loaded into python).  The program needs the host compiler
and csrc's headers only, so this test compiles it itself (a few seconds), into pytest's temporary directory."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "add_affine_test.cpp")
CSRC = os.path.join(ROOT, "crypto3-zk_amd", "csrc")
FIELDS = ("BLS12-381 Fq", "BN254 Fq", "Pallas Fq", "Vesta Fq")


def _build(exe, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-I", CSRC, *flags, SRC, "-o", str(exe)])
    return str(exe)


def _check(exe, env=None):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, text=True, env=env)
    assert out.returncode == 0, out.stdout[-4000:]
    for f in FIELDS:
        line = next(l for l in out.stdout.splitlines() if l.startswith(f + ":"))
        checks, mismatches = int(line.split()[-4]), int(line.split()[-2])
        assert mismatches == 0 and checks >= 4000 + 625, line
    return out.stdout


def test_add_affine_equals_madd_of_from_affine(tmp_path):
    _check(_build(tmp_path / "add_affine_test", "-O2"))


def test_add_affine_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path / "add_affine_test_san", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    log = _check(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "AddressSanitizer" not in log and "runtime error" not in log and "LeakSanitizer" not in log, log[-4000:]
