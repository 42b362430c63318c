"""The entries stage after its launch chain was cut (csrc/msm_entries.hip: one two-barrier LDS scan, scans in two launches, the size
histogram counted by the sort's final pass, the large-bucket plan written by the size sort's last kernel, a third tile shape).

tests/cpp/scantest.hip runs the scan primitive by itself; tests/cpp/entries_latency_test.hip runs tests/cpp/entriestest.hip's own checks
(test_gpu_msm_entries.py: every buffer of the stage against a host restatement) over the sizes at the wave, workgroup and tile boundaries
of the three tile shapes, the two-launch scans, the merged plan, narrow super-buckets, and compares two runs of one input.  Each
program runs once; the tests below read their parts of its output.  The MSMs over the same shapes are compared with the oracle as in
test_gpu_msm.py."""
import subprocess

import numpy as np
import pytest

import cport as cp
from harness import program

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 1023, 1025, 2 ** 13 - 1, 2 ** 13 + 1, 2 ** 14 + 1)
TILE_LOGS = (12, 13, 14)
N = 3000  # points of the MSMs below: above the 128-entry split threshold when all scalars are equal, one tile of every shape


def run_program(name):
    out = subprocess.run([program(name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    return out.returncode, out.stdout


@pytest.fixture(scope="module")
def stage():
    """(exit code, output lines) of entries_latency_test"""
    rc, text = run_program("entries_latency_test")
    return rc, text.splitlines()


def lines_of(stage, prefix, count):
    rc, lines = stage
    mine = [ln for ln in lines if ln.startswith(prefix)]
    assert len(mine) == count and all(": ok (" in ln for ln in mine), "\n".join(mine or lines)
    return mine


def test_scan_primitive():
    rc, text = run_program("scantest")
    assert rc == 0 and text.count(": ok (") == 10, text  # five inputs x {256, 1024} lanes


def test_stage_buffers_at_wave_workgroup_and_tile_boundaries(stage):
    got = lines_of(stage, "sizes: ", len(SIZES) * len(TILE_LOGS))
    assert [ln.split(":")[1].strip() for ln in got] == ["n = %d, tile log %d" % (n, t) for t in TILE_LOGS for n in SIZES]


def test_two_launch_scans(stage):
    (ln,) = lines_of(stage, "scan: ", 1)
    assert "512 super-buckets, 11 tiles" in ln and "13 windows of 13" in ln and "1 sets x 524288 buckets" in ln  # 73 216 and 66 560 counters


def test_merged_large_plan(stage):
    got = lines_of(stage, "plan: ", 4)
    assert sum("0 large buckets in 0 tasks" in ln for ln in got) == 1  # the zero scalars alone
    assert all("0 large buckets" not in ln.replace("0 large buckets in 0 tasks", "") or "zero scalars" in ln for ln in got)


def test_narrow_super_buckets(stage):
    lines_of(stage, "narrow: ", 4)


def test_two_runs_agree(stage):
    lines_of(stage, "twice: ", 3)
    assert stage[0] == 0, "\n".join(stage[1])


@pytest.fixture(scope="module")
def points():
    pts, _ = cp.batch_mul(0, 1, cp.random_fr(0, 71, N))
    return pts


def check_msm(ctx, pts, scalars, options):
    """the MSM under `options` against the oracle; no kernel may have raised a status flag (a large-bucket plan beyond its capacity is one)"""
    exp, einf = cp.msm(0, 1, pts, scalars, chunks=4)
    try:
        for name, v in options.items():
            ctx.set_option(name, v)
        bases = ctx.upload_bases(0, 1, pts)  # window tables for this c
        aff, inf = ctx.msm_affine(bases, scalars)
        assert ctx.device_status() == 0
        bases.free()
    finally:
        for name, v in (("msm_window_bits", 0), ("msm_sets", 0), ("msm_sort_tile_log", 14)):
            ctx.set_option(name, v)
    assert inf == einf and (aff == exp).all(), options


@pytest.mark.parametrize("c,tile_log", [(11, 13), (20, 14), (8, 12)])
def test_msm_equal_scalars_matches_oracle(ctx, points, c, tile_log):
    """every window has one bucket above the split threshold: the plan written by msm_size_scatter drives msm_bucket_large"""
    scalars = np.repeat(cp.random_fr(0, 72, 1), N, axis=0)
    check_msm(ctx, points, scalars, {"msm_window_bits": c, "msm_sort_tile_log": tile_log})


def test_msm_zero_scalars_matches_oracle(ctx, points):
    """every digit is DIG_NONE: no entry, no large bucket, the sum is the point at infinity"""
    check_msm(ctx, points, np.zeros((N, 4), dtype=np.uint64), {"msm_window_bits": 11, "msm_sort_tile_log": 13})


@pytest.mark.parametrize("c,sets,tile_log", [(8, 3, 12), (8, 3, 13), (5, 7, 14), (10, 2, 13)])
def test_msm_narrow_super_buckets_matches_oracle(ctx, points, c, sets, tile_log):
    """2^(c - 1) < 1024 buckets per super-bucket, several sets: msm_size_hist counts the sizes"""
    check_msm(ctx, points, cp.random_fr(0, 73, N), {"msm_window_bits": c, "msm_sets": sets, "msm_sort_tile_log": tile_log})


@pytest.mark.parametrize("tile_log", TILE_LOGS)
def test_msm_wide_super_buckets_matches_oracle(ctx, points, tile_log):
    """c = 20: 512 super-buckets of 1024 buckets, the final pass counts the sizes, the size sort's scan takes two launches"""
    check_msm(ctx, points, cp.random_fr(0, 74, N), {"msm_window_bits": 20, "msm_sort_tile_log": tile_log})
