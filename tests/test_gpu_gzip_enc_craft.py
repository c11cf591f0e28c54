"""Directed payloads through the GPU gzip encoder (zcg_deflate.hip): zlib's
bytes, at every level a case runs at.

zlib inflating a member says that the member is right; the generic payloads
of test_gpu_encode.py do not decide which branches of the GPU-only code wrote
it.  The batches of tests/gz_enc_cases.py are built to reach them: the window
and MAX_DIST rules, the prefix compares and the chain budgets of
dz_search_run, the stitch of dz_parse (empty tails, skipped segments, the
tail cap on both sides, the serial fallback), the block cuts, the register
window, LDS ring and max_insert rule of dz_parse_fast, length-limited trees,
the code-length run coding, stored blocks between blocks that start inside a
byte.  Each has a witness asserted on the CPU
(tests/test_gz_enc_cases_host.py).  Here each (case, level) is one
zcg_encode_batch call over the case's chunks, and every member must pass
check_gzip_member(exact=True): header, CRC32 / ISIZE, zlib inflates it, and
the deflate body equals zlib's; a difference is reported by block, symbol and
input position.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

zref = pytest.importorskip("zref")

import gz_enc_cases as ec  # noqa: E402
from golden_util import dtype_info  # noqa: E402
from gpu_check import check_gzip_member, encode_batch, meta_for  # noqa: E402


@pytest.mark.parametrize("name,level", ec.RUNS, ids=[f"{n}-{lv}" for n, lv in ec.RUNS])
def test_case(name, level):
    c = ec.case(name)
    es = dtype_info(c.dt)[0]
    assert c.D % es == 0
    meta = meta_for("gzip", c.dt, c.D // es, level)
    arrays = [np.frombuffer(x, np.uint8) for x in c.native()]
    st, outs = encode_batch(meta, arrays)
    assert (st == 0).all(), (name, level, st.tolist())
    for i, (s, content) in enumerate(zip(outs, c.chunks)):
        try:
            check_gzip_member(s, content, level, exact=True)
        except AssertionError as e:
            raise AssertionError(f"{name} level {level} chunk {i}: {e}") from e
