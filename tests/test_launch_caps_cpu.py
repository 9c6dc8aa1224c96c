"""tests/launch_caps.py held to the launchers it was read from, and the conditions tests/test_launch_shape_gpu.py relies on that the
reference alone decides -- all without a GPU.

Every formula of launch_caps.py restates one expression of a launcher.  Each test below finds that expression in the launcher's own
body and fails, naming launch_caps.py, when the line no longer reads so: a raised (or re-shaped) cap then fails here instead of
silently turning the GPU cases back into single-trip tests.  (tests/test_capi_cpu.py parses scn_mixed_plans.h the same way.)"""
import os

import numpy as np
import pytest

from tests import launch_caps as caps
from tests import tolerances as tol

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scanner_amd", "csrc")


def _body(fname, signature):
    """the text of the function whose definition starts with `signature`, from there to its closing brace in column 0"""
    with open(os.path.join(CSRC, fname)) as fh:
        src = fh.read()
    assert src.count(signature) == 1, f"{fname}: `{signature}` occurs {src.count(signature)} times -- tests/launch_caps.py was read from one definition"
    start = src.index(signature)
    end = src.index("\n}", start)
    return src[start:end]


def _reads(body, expr, what, fname):
    assert expr in body, (f"{fname}: {what} no longer reads `{expr}` -- restate it in tests/launch_caps.py (and in this test), so that "
                          f"tests/test_launch_shape_gpu.py still takes every workgroup through its loop twice")


def test_four_step_columns_cap():
    f = "scn_big.hip"
    body = _body(f, "hipError_t scn_launch_big(")
    _reads(body, "const uint32_t ct = n / 4096u;", "the number of column tiles", f)
    _reads(body, "uint32_t G = (uint32_t)(num_cus * 3) / ct;", "the column kernel's buffers per trip", f)
    _reads(body, "if (G < 1) G = 1;", "the lower bound of G", f)
    _reads(body, "launch_cols<BN>(kind, dc, a, ct * G, lds, s) : launch_cols<32768u>(kind, dc, a, ct * G, lds, s)", "the column kernel's grid", f)
    kernel = _body(f, "__global__ __launch_bounds__(256, 3) void scn_big_cols_kernel(")
    _reads(kernel, "G = gridDim.x / CT;", "the column kernel's own G", f)
    _reads(kernel, "for (uint32_t b = g; b < args.n_buffers; b += G) {", "the column kernel's buffer loop", f)
    assert (caps.FOUR_STEP_TILE, caps.FOUR_STEP_WG_PER_CU) == (4096, 3)
    assert caps.four_step_cap(256, 32768) == 96 and caps.four_step_cap(256, 65536) == 48
    assert caps.four_step_cap(2, 65536) == 1   # (the launcher's lower bound)
    assert caps.two_trips_and(caps.four_step_cap(256, 32768), 5) == 197 and caps.two_trips_and(caps.four_step_cap(256, 65536), 5) == 101


def test_bluestein_caps():
    f = "scn_generic.hip"
    body = _body(f, "hipError_t scn_launch_generic(")
    _reads(body, "const int resident = num_cus * 8;", "the resident workgroups", f)
    _reads(body, "const int load_grid = (int)((uint32_t)resident < a.n_buffers ? (uint32_t)resident : a.n_buffers);", "the load kernel's grid", f)
    _reads(body, "size_t b = (items + 255u) / 256u;", "the items per block", f)
    _reads(body, "const size_t cap = (size_t)resident * 4u;", "the block cap of the stage, pointwise and finish kernels", f)
    _reads(body, "return (int)(b < cap ? b : cap);", "the block cap's use", f)
    for r in (2, 4, 16):
        _reads(body, f"(scn_gen_stage_kernel<{r}>), dim3(blocks_for((size_t)a.m / {r} * a.n_buffers)), dim3(256)", f"the radix-{r} stage's grid", f)
    _reads(body, "scn_gen_pointwise_kernel, dim3(blocks_for((size_t)a.m * a.n_buffers)), dim3(256)", "the pointwise kernel's grid", f)
    _reads(body, "const int fin = blocks_for((size_t)a.n * a.n_buffers);", "the finish kernel's grid", f)
    _reads(body, "if (a.log2m & 1u) {", "the radix-2 stage's condition", f)
    _reads(body, "if (a.log2m & 2u) {", "the radix-4 stage's condition", f)
    with open(os.path.join(CSRC, "scn_host.hip")) as fh:
        _reads(fh.read(), "for (t.log2m = 0; (1u << t.log2m) < 2u * n - 1u; t.log2m++) {", "the convolution length", "scn_host.hip")
    with open(os.path.join(CSRC, f)) as fh:
        src = fh.read()
    assert src.count("g += (size_t)gridDim.x * 256u)") == 3, f"{f}: the stage, pointwise and finish loops no longer advance by gridDim.x * 256 -- tests/launch_caps.py"
    _reads(src, "for (uint32_t b = blockIdx.x; b < a.n_buffers; b += gridDim.x) {", "the load kernel's buffer loop", f)
    assert (caps.GEN_RESIDENT_PER_CU, caps.GEN_BLOCKS_PER_RESIDENT, caps.GEN_THREADS) == (8, 4, 256)
    assert caps.bluestein_load_cap(256) == 2048 and caps.bluestein_item_cap(256) == 2097152 == 8192 * 256
    assert caps.bluestein_m(11000) == 32768 and caps.bluestein_m(17) == 64 and caps.bluestein_m(65535) == 131072 and caps.bluestein_m(16385) == 65536
    assert caps.bluestein_radices(11000) == [2, 4, 16, 16, 16] and caps.bluestein_radices(17) == [4, 16] and caps.bluestein_radices(65535) == [2, 16, 16, 16, 16]
    # 11000 points: every radix, and the kernel with the fewest items per buffer is the radix-16 stage (2048 of them)
    assert caps.bluestein_items(11000, 1) == {"stage<2>": 16384, "stage<4>": 8192, "stage<16>": 2048, "pointwise": 32768, "finish": 11000}
    for cus in (256, 64, 32, 304):
        cap = caps.bluestein_stage_cap(cus, 11000)
        assert cap == 4 * cus
        nb = caps.two_trips_and(cap, 7)
        assert nb == 8 * cus + 7
        assert all(items > 2 * caps.bluestein_item_cap(cus) for items in caps.bluestein_items(11000, nb).values())
        # the fallback batch of the GPU test (4 CUs + 7) still loops every kernel once
        assert all(items > caps.bluestein_item_cap(cus) for items in caps.bluestein_items(11000, cap + 7).values())


def test_signal_and_scan_caps():
    f = "scn_hits.hip"
    geo = _body(f, "static void signal_geometry(")
    _reads(geo, "a.map_words = (3u * words + 1u) & ~1u;", "the three maps' words", f)
    _reads(geo, "const uint32_t most = (((a.n + 1u) / 2u) + 63u) & ~63u;", "the signals a unit can have", f)
    _reads(geo, "uint32_t w = 4u, chunk = 0;", "the largest wave count", f)
    _reads(geo, "const uint32_t budget = (48u * 1024u / 4u) / w;", "the 48 KiB budget", f)
    _reads(geo, "chunk = budget > a.map_words ? ((budget - a.map_words) / 5u) & ~63u : 0u;", "the chunk", f)
    _reads(geo, "if (chunk >= (most < 256u ? most : 256u) || w == 1u) break;", "the choice of the wave count", f)
    for fn, kernel in (("scn_launch_signal_count", "scn_signal_count_kernel"), ("scn_launch_signal_build", "scn_signal_build_kernel")):
        body = _body(f, f"hipError_t {fn}(")
        _reads(body, "uint32_t blocks = (a.n_buffers + waves - 1u) / waves;", f"{fn}'s blocks", f)
        _reads(body, "if (blocks > 8192u) blocks = 8192u;", f"{fn}'s block cap", f)
        _reads(body, f"{kernel}, dim3(blocks), dim3(64u * waves)", f"{fn}'s launch", f)
        k = _body(f, f"__global__ __launch_bounds__(256) void {kernel}(")
        _reads(k, "for (uint32_t b = blockIdx.x * waves + wave; b < a.n_buffers; b += gridDim.x * waves) {", f"{kernel}'s unit loop", f)
    with open(os.path.join(CSRC, f)) as fh:
        src = fh.read()
    _reads(src, "constexpr uint32_t kScanThreads = 256;", "the scan's threads", f)
    _reads(src, "constexpr uint32_t kScanChunk = kScanThreads * 8u;", "the scan's counts per workgroup", f)
    _reads(_body(f, "hipError_t scn_launch_hit_scan("), "(a.n_buffers + kScanChunk - 1u) / kScanChunk", "the scan's grid", f)
    assert (caps.SIGNAL_LDS_BYTES, caps.SIGNAL_MAX_BLOCKS, caps.SCAN_CHUNK) == (49152, 8192, 2048)
    # 4 waves while the maps and 256 signals' state fit a quarter of 48 KiB: (12288 / 4 - 3 n / 32) / 5 >= 256, n <= 19093 or so
    assert [caps.signal_waves(n) for n in (16, 64, 1000, 4096, 16384)] == [4, 4, 4, 4, 4]
    assert caps.signal_waves(32768) == 2 and caps.signal_waves(65536) == 1   # (test_signals_gpu.py: two waves per workgroup at 32768)
    assert caps.signal_cap(64) == 32768
    nb = caps.two_trips_and(caps.signal_cap(64), 19)
    assert nb == 65555 and -(-nb // caps.SCAN_CHUNK) == 33


def test_convert_cap():
    f = "scn_kernels.hip"
    body = _body(f, "hipError_t scn_launch_convert(")
    _reads(body, "dim3(n_buffers < 2048 ? n_buffers : 2048), dim3(256)", "the convert kernel's grid", f)
    kernel = _body(f, "__global__ __launch_bounds__(256) void scn_convert_kernel(")
    _reads(kernel, "for (uint32_t buf = blockIdx.x; buf < n_buffers; buf += gridDim.x) {", "the convert kernel's buffer loop", f)
    assert caps.convert_cap() == 2048 and caps.two_trips_and(caps.convert_cap(), 13) == 4109


def test_trips():
    cap = 96
    nb = caps.two_trips_and(cap, 5)
    trips = np.bincount([caps.trip_of(b, cap) for b in range(nb)])
    assert trips.tolist() == [96, 96, 5]
    with pytest.raises(AssertionError):
        caps.two_trips_and(cap, 4)
    # few CUs: the remainder shrinks below the cap, the batch still exceeds twice the cap (G = 3 at 16 CUs and 65536 points)
    assert [caps.two_trips_and(c, 5) for c in (1, 2, 3, 5, 6)] == [3, 5, 7, 13, 17]
    assert all(caps.two_trips_and(caps.four_step_cap(cus, 65536), 5) > 2 * caps.four_step_cap(cus, 65536) for cus in range(1, 40))


# ---- what the GPU shapes rely on and the reference alone decides ----------------------------------------------------------------
@pytest.mark.parametrize("n,nb", [(11000, 96), (65536, 24)])
def test_exempt_share_and_distinct_counts_of_the_float64_referenced_shapes(oracle_mod, n, nb):
    """The two float64-referenced GPU cases demand the records exactly wherever the spectrum bar could not move the bin across the
    threshold (tol.flip_unsafe) and allow at most MAX_EXEMPT_SHARE = 2 % of the reference's records to be exempt.  A CPU sample
    of the same generator, window and threshold rule: the share stays under that cap (measured 0.35 % at 11000 points, 0.45 % at
    65536), and the per-buffer hit counts take more than 10 distinct values -- a skipped, repeated or swapped buffer cannot
    hide behind equal counts."""
    x = caps.scene(n, nb, seed=7000 + n)
    db = caps.float64_db(x, oracle_mod.Oracle(n).window())
    ev = tol.evaluated_mask(n)
    thr = caps.noise_tail_threshold(db, ev)
    b, i = caps.reference_hits(db, thr, ev, n)
    share = caps.exempt_share(db, thr, ev, n, tol.flip_unsafe(db, thr))
    counts = np.bincount(b, minlength=nb)
    rate = len(b) / (nb * ev.sum())
    print(f"n {n}: {nb} buffers, threshold {thr:.3f} dB, {len(b)} records ({1e3 * rate:.2f} per thousand evaluated bins), exempt share "
          f"{100 * share:.3f} %, {len(np.unique(counts))} distinct per-buffer counts ({counts.min()} .. {counts.max()})")
    assert share < caps.MAX_EXEMPT_SHARE, (share, caps.MAX_EXEMPT_SHARE)
    assert len(np.unique(counts)) > 10, np.unique(counts)
    assert 5e-4 < rate < 2e-2, rate
