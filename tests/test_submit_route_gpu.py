"""The one route the GPU suite's shapes never took: a transform that is not fused (a floor plan; a Bluestein plan) on the plan's shared
stream, whose previous collect took records -- so the list is built behind the launch, on the list stream -- with 2^18 units or more
(submit_route, scanner_amd/csrc/scn_host.hip: the counts go by DMA there, not by the reduction, which records no event for the list
stream to wait on).  The reference is the same plan on the same input in two halves below 2^18 units, routes the suite holds
elsewhere: the whole submit's records must be those of the halves byte for byte and its trigger bytes equal, twice, so that both
generations of the hit outputs carry it."""
import numpy as np
import pytest
import torch

from scanner_amd import Plan, capi
from tests import tolerances as tol
from tests.test_floor_gpu import _straddling

pytestmark = pytest.mark.gpu

FS = 8000000
UNITS = (1 << 18) + 37
HALF = 1 << 17


# (3.0 over the median of noise that straddles 0 dB is the Rayleigh tail of 1 / 16, for the floor plan over its unit's floor and for the
#  fixed threshold over 0 dB alike)
@pytest.mark.parametrize("n,detect", [(16, capi.DETECT_FLOOR), (17, capi.DETECT_FIXED)])
def test_whole_submit_equals_its_halves(built_lib, n, detect):
    kept = int(tol.evaluated_mask(n).sum())
    cap = UNITS * kept // 4  # four times the expected 1 / 16 of the evaluated bins: nothing is truncated
    x = _straddling(n, UNITS, seed=n)
    d_raw = torch.from_numpy(x.view(np.uint8).reshape(-1)).cuda()
    fc = 100e6 + 6e6 * np.arange(UNITS)
    seq = 1000 + 3 * np.arange(UNITS, dtype=np.uint64)
    out = np.empty(cap, capi.HIT_DTYPE)
    with Plan(n, FS, 3.0, max_batch=UNITS, max_hits=cap, flags=capi.OUT_HITS, detect=detect, trigger_count=1) as plan:
        def run(lo, hi):
            plan.submit_device(0, d_raw[lo * plan.buffer_bytes:], hi - lo, center_freqs=fc[lo:hi], seq_ids=seq[lo:hi])
            _, h, t = plan.collect(0, hits_out=out)
            assert len(h) == plan.last_n_hits < cap
            return h.tobytes(), t.copy()

        (h0, t0), (h1, t1) = run(0, HALF), run(HALF, UNITS)  # counts only wanted so far; then eager, below 2^18 units
        want_h, want_t = h0 + h1, np.concatenate([t0, t1])
        total = len(want_h) // capi.HIT_DTYPE.itemsize
        assert UNITS * kept // 64 < total < cap and 0 < int(want_t.sum()) < UNITS, (total, int(want_t.sum()))
        for rep in range(2):  # eager, from 2^18 units: the route in question, once per generation
            got_h, got_t = run(0, UNITS)
            assert got_h == want_h, f"submit {rep}: the whole submit's records differ from the halves'"
            assert np.array_equal(got_t, want_t), f"submit {rep}: the trigger bytes differ"
