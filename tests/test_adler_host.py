"""The Adler-32 arithmetic of the GPU kernels (zarr_amd/csrc/zcg_adler.h) on
the CPU: tests/adler_host walks a file's bytes the way adler32_verify's waves,
zlib_adler32's workgroup and a single lane at the deferred-modulo bound do, and
the result must be zlib.adler32's.  The program is built with
-fsanitize=address,undefined and runs on its own."""
import os
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "adler_host")
LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 5552, 5553, 65521, (1 << 20) + 3]


@pytest.fixture(scope="module")
def prog():
    subprocess.run(["make", "-C", DIR], check=True, capture_output=True)
    with open(os.path.join(DIR, "Makefile")) as f:
        assert "-fsanitize=address,undefined" in f.read()
    return os.path.join(DIR, "adler_host")


def run(prog, mode, path):
    r = subprocess.run([prog, mode, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout, 16)


def patterns(n):
    rng = np.random.default_rng(n)
    yield "random", rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    yield "ramp", (np.arange(n) % 251).astype(np.uint8).tobytes()
    yield "ff", b"\xff" * n


@pytest.mark.parametrize("n", LENGTHS)
def test_lane_arithmetic_and_fold_equal_zlib(prog, tmp_path, n):
    for name, data in patterns(n):
        p = tmp_path / name
        p.write_bytes(data)
        want = zlib.adler32(data)
        for mode in ("comb", "block", "lane"):
            assert run(prog, mode, str(p)) == want, (n, name, mode)


def test_4_mib_of_ff(prog, tmp_path):
    data = b"\xff" * (4 << 20)
    p = tmp_path / "ff"
    p.write_bytes(data)
    for mode in ("comb", "block", "lane"):
        assert run(prog, mode, str(p)) == zlib.adler32(data), mode


def test_one_lane_past_the_deferred_modulo_bound(prog, tmp_path):
    """ADLER_LANE_MAX_PIECES = 1 052 688 pieces of 0xFF (16 843 008 bytes) fill a
    lane's 32-bit byte sum; 'lane' mode closes the lane there and goes on."""
    bound = 1052688 * 16
    for n in (bound - 1, bound, bound + 1, bound + 17):
        data = b"\xff" * n
        p = tmp_path / "ff"
        p.write_bytes(data)
        assert run(prog, "lane", str(p)) == zlib.adler32(data), n
