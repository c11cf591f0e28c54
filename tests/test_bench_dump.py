"""bench.py --dump-outputs on the CPU: the files dump_outputs writes from a
decoded batch (the sample is fixed, the types are float32/float64, the byte
sums cover every chunk) and the plain / --full split of the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(n, D, seed):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(seed)
    host = rng.integers(-300, 300, n * D // 2).astype("<i2")
    dst = torch.from_numpy(host.view(np.uint8).copy())
    status = torch.zeros(n, dtype=torch.int32)
    status[3] = -7
    return host.reshape(n, D // 2), dst, status


@pytest.mark.parametrize("n", [5, 300])  # fewer chunks than the sample; more than one 256-chunk slice
def test_dump_outputs_files(tmp_path, n):
    import bench
    D = 64
    host, dst, status = _batch(n, D, 1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), np.dtype("<i2"), dst, status, n, D, 0, 1)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["chunk_byte_sums.npy", "decoded.npy", "decoded_rows.npy", "status.npy"]
    got = {f: np.load(tmp_path / "a" / f) for f in names}
    for f in names:  # same arguments, same files
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f))
        assert got[f].dtype in (np.float32, np.float64)
    rows = got["decoded_rows.npy"].astype(np.int64)
    assert len(rows) == min(n, bench.DUMP_CHUNKS) and len(set(rows)) == len(rows)
    assert np.array_equal(got["decoded.npy"], host[rows].astype(np.float32))
    assert np.array_equal(got["status.npy"], status.numpy().astype(np.float32))
    assert np.array_equal(got["chunk_byte_sums.npy"],
                          host.view(np.uint8).reshape(n, D).sum(axis=1, dtype=np.int64).astype(np.float64))


def test_dump_sample_fits_the_size_limit():
    import bench
    # the widest expansion is i16 -> float32 (x2) of 1 MiB chunks
    assert bench.DUMP_CHUNKS * (1 << 20) * 2 + 65536 * 3 * 8 <= 64 * 1000 * 1000


def test_dump_outputs_rank_suffix(tmp_path):
    import bench
    _, dst, status = _batch(4, 16, 2)
    bench.dump_outputs(str(tmp_path), np.dtype("<i2"), dst, status, 4, 16, 1, 2)
    assert sorted(os.listdir(tmp_path)) == ["chunk_byte_sums_rank1.npy", "decoded_rank1.npy",
                                            "decoded_rows_rank1.npy", "status_rank1.npy"]


def test_cli_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True)
    assert r.returncode == 2 and "--steps" in r.stderr
