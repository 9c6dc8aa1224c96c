"""The grid caps of the launchers whose kernels walk the rest of their work in a `for (...; x += stride)` loop, each as a small
function of the CU count (and of n where it matters), and the batch that takes every workgroup of such a kernel through its loop
TWICE, with a ragged remainder on a third trip.  tests/test_launch_shape_gpu.py sizes every case from here;
tests/test_launch_caps_cpu.py holds every formula to the line of the launcher it was read from, so that a raised cap fails on a CPU
instead of silently turning the GPU cases back into single-trip tests.

  kernel                                               launcher (file)                          workgroups
  scn_big_cols_kernel, 32768 / 65536 points            scn_launch_big (scn_big.hip)             ct * G, G = max(1, 3 CUs / ct), ct = n / 4096;
                                                                                                workgroup (j, g) takes buffers g, g + G, ...
  scn_gen_load_kernel                                  scn_launch_generic (scn_generic.hip)     min(8 CUs, n_buffers), one buffer per trip
  scn_gen_stage_kernel<2 / 4 / 16>, _pointwise, _finish  the same, blocks_for                   min(ceil(items / 256), 32 CUs) of 256 threads,
                                                                                                one item per thread and trip
  scn_signal_count_kernel, scn_signal_build_kernel     scn_launch_signal_* (scn_hits.hip)       min(ceil(units / waves), 8192), one unit per wave
                                                                                                and trip; waves from signal_geometry
  scn_hit_scan_kernel                                  scn_launch_hit_scan (scn_hits.hip)       one per 2048 counts (no cap: every further
                                                                                                workgroup sums the chunks before its own)
  scn_convert_kernel                                   scn_launch_convert (scn_kernels.hip)     min(n_buffers, 2048), one buffer per trip
"""
import numpy as np

from scanner_amd import synth

# ---- scn_big.hip, scn_launch_big ------------------------------------------------------------------------------------------------
FOUR_STEP_TILE = 4096        # `const uint32_t ct = n / 4096u;`
FOUR_STEP_WG_PER_CU = 3      # `uint32_t G = (uint32_t)(num_cus * 3) / ct;`


def four_step_cap(num_cus, n):
    """G: the buffers one trip of the column kernel's loop takes (workgroup (j, g) owns tile j of buffers g, g + G, ...)"""
    assert n in (32768, 65536)
    return max(1, (num_cus * FOUR_STEP_WG_PER_CU) // (n // FOUR_STEP_TILE))


# ---- scn_generic.hip, scn_launch_generic ----------------------------------------------------------------------------------------
GEN_RESIDENT_PER_CU = 8      # `const int resident = num_cus * 8;`
GEN_BLOCKS_PER_RESIDENT = 4  # `const size_t cap = (size_t)resident * 4u;`
GEN_THREADS = 256            # `(items + 255u) / 256u`, dim3(256)


def bluestein_load_cap(num_cus):
    """buffers per trip of scn_gen_load_kernel: one per workgroup"""
    return num_cus * GEN_RESIDENT_PER_CU


def bluestein_item_cap(num_cus):
    """items per trip of the stage, pointwise and finish kernels: one per thread (8192 per CU)"""
    return num_cus * GEN_RESIDENT_PER_CU * GEN_BLOCKS_PER_RESIDENT * GEN_THREADS


def bluestein_m(n):
    """the convolution length: the power of two >= 2 n - 1"""
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def bluestein_radices(n):
    """the stage radices of one transform of length M, in launch order: log2 M = 4 s + r, one radix-2 stage if r is odd, one radix-4
    stage if r >= 2, radix 16 from there on"""
    log2m = bluestein_m(n).bit_length() - 1
    out = ([2] if log2m & 1 else []) + ([4] if log2m & 2 else [])
    return out + [16] * ((log2m - (log2m & 3)) // 4)


def bluestein_items(n, nb):
    """items of every looping kernel of a launch of nb n-point buffers: {kernel: items}"""
    m = bluestein_m(n)
    out = {f"stage<{r}>": (m // r) * nb for r in set(bluestein_radices(n))}
    out["pointwise"] = m * nb
    out["finish"] = n * nb
    return out


def bluestein_stage_cap(num_cus, n):
    """buffers per trip of the kernel with the FEWEST items per buffer (M / 16 for the radix-16 stage): a batch of more than
    twice this many takes every thread of every stage, of the pointwise and of the finish kernel through its loop at least twice"""
    per_buffer = min(v for v in bluestein_items(n, 1).values())
    cap = bluestein_item_cap(num_cus)
    assert cap % per_buffer == 0
    return cap // per_buffer


# ---- scn_hits.hip ---------------------------------------------------------------------------------------------------------------
SIGNAL_LDS_BYTES = 48 * 1024   # `const uint32_t budget = (48u * 1024u / 4u) / w;`
SIGNAL_MAX_BLOCKS = 8192       # `if (blocks > 8192u) blocks = 8192u;`
SCAN_CHUNK = 256 * 8           # kScanThreads * 8u counts per workgroup of scn_hit_scan_kernel


def signal_waves(n):
    """signal_geometry written out: the most waves per workgroup (4, 2, 1) whose share of 48 KiB of LDS holds the unit's three maps
    and the state of at least min(256, signals a unit can have) signals, 5 words each"""
    words = (n + 31) // 32
    map_words = (3 * words + 1) & ~1
    most = (((n + 1) // 2) + 63) & ~63
    w = 4
    while True:
        budget = (SIGNAL_LDS_BYTES // 4) // w
        chunk = ((budget - map_words) // 5) & ~63 if budget > map_words else 0
        if chunk >= min(most, 256) or w == 1:
            return w
        w >>= 1


def signal_cap(n):
    """units per trip of the signal kernels: one per wave of 8192 workgroups"""
    return SIGNAL_MAX_BLOCKS * signal_waves(n)


# ---- scn_kernels.hip, scn_launch_convert ----------------------------------------------------------------------------------------
CONVERT_MAX_BLOCKS = 2048      # `dim3(n_buffers < 2048 ? n_buffers : 2048)`


def convert_cap():
    return CONVERT_MAX_BLOCKS


# ---- batches --------------------------------------------------------------------------------------------------------------------
def two_trips_and(cap, rest):
    """twice the cap plus a small odd remainder: `rest` workgroups (buffers, units) make three trips, the others two.  Where the cap
    is no larger than `rest` (a partition of very few CUs) the remainder shrinks to the largest odd number below the cap, 1 at the
    least: the batch stays a two-trip one with a ragged third trip (at a cap of 1, three trips of the one workgroup)."""
    assert rest % 2 == 1 and rest > 0 and cap >= 1
    while rest >= cap and rest > 1:
        rest -= 2
    return 2 * cap + rest


def trip_of(index, cap):
    """the trip of its workgroup's loop on which item `index` is taken (0: the first): the loops advance by exactly the grid"""
    return index // cap


# ---- the float64-referenced shapes: generator, threshold and the share of records the spectrum bar itself could move ------------
def scene(n, nb, seed):
    """every buffer its own noise and its own tones (synth.cfloat_batch: 0 .. 4 tones at random fractional bins and levels)"""
    return synth.cfloat_batch(n, nb, seed=seed, sigma=0.05)


def float64_db(x, window_f32, chunk=256):
    """The plain float64 reference: x * window in float32 (as the kernels and the reference multiply floats), numpy's FFT in
    complex128, 5 log10 |X|^2.  float64 [B, n]"""
    w = np.asarray(window_f32, np.float32)
    out = np.empty(x.shape, np.float64)
    for lo in range(0, len(x), chunk):
        xw = x[lo:lo + chunk]
        xw = (xw.real * w + 1j * (xw.imag * w)).astype(np.complex64)  # two float32 products per sample
        X = np.fft.fft(xw.astype(np.complex128), axis=-1)
        with np.errstate(divide="ignore"):
            out[lo:lo + chunk] = 5.0 * np.log10(X.real ** 2 + X.imag ** 2)
    return out


def noise_tail_threshold(db, ev):
    """the median of the evaluated bins + 5 dB, a float32 (a noise bin's power is exponentially distributed: about two bins per
    thousand lie above it)"""
    return float(np.float32(np.median(db[:, ev]) + 5.0))


MAX_EXEMPT_SHARE = 0.02   # of the reference's records


def reference_hits(db, thr, ev, n):
    """(buffer [H], i [H]) ordered by (buffer, i): the evaluated bins of a float64 spectrum strictly above thr (process.cpp:46-62:
    i walks the fftshift order, natural bin j = (i + n / 2) % n)"""
    i = np.arange(n)
    j = (i + n // 2) % n
    hit = (db[:, j] > thr) & ev[j][None, :]
    b, ii = np.nonzero(hit)
    return b, ii


def exempt_share(db, thr, ev, n, unsafe):
    """the share of the reference's records that sit on a bin the spectrum tolerance itself could move across thr"""
    b, i = reference_hits(db, thr, ev, n)
    return float(unsafe[b, (i + n // 2) % n].mean()) if len(b) else 0.0
