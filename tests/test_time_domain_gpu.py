"""Time-domain mode (process.cpp:203-237, the CLI's default mode) held to every sample, launch shape and special value: the two
kernels of scanner_amd/csrc/scn_kernels.hip -- scn_time_domain_wave_kernel (one wave per buffer, 16-byte loads, n % 8 == 0) and
scn_time_domain_kernel (one workgroup per buffer, every other n) -- against the plain reference of tests/td_scenes.py on scenes whose
maximum and minimum are PLANTED samples, at least 1 dB clear of every other sample (tests/test_td_scenes_cpu.py asserts that of the
reference alone).  tests/test_parity_gpu.py test_time_domain_mode cannot see a dropped sample: its samples lie below 0 dB, where the
reference's maximum is the clamp constant, and its strong sample sits at index 17.

  * test_every_sample_counts: n buffers of n samples, the maximum planted at sample b of buffer b and the minimum at n - 1 - b, at
    every size at which a loop bound is crossed; with DC removal off the results are bit-identical across the buffers (the kernels
    reduce p exactly and convert once), so a dropped position is a whole-dB outlier;
  * test_more_buffers_than_resident_waves: more than twice the buffers the capped grid holds, levels that are functions of the
    buffer index (a stride or indexing error swaps different levels); `above` exactly mx >= threshold at a threshold that IS one of
    the levels;
  * test_long_buffers: 2^20 samples in every format (with DC removal the int16 sum wraps to 0), 2^24 in int8;
  * test_special_values: NaN, +-inf, zeros, denormal powers, a power that overflows, one near FLT_MAX, in both kernel forms;
  * test_above_flag_on_the_knife_edge.
Bars: 1e-4 dB on the maximum and 2e-3 dB on the minimum (test_time_domain_mode's); +-inf and the clamp constants compare exactly.

MODULE STATE: the figures are a module global filled in test order; test_zz_figures prints the table (run with -rP or -s) and
asserts that every (kernel form, format) pair was seen only where the whole module ran."""
import numpy as np
import pytest

from scanner_amd import Plan, build, capi
from tests import td_scenes as sc

pytestmark = pytest.mark.gpu
FS = 8000000
WAVE_SIZES = [8, 16, 24, 64, 512, 520, 1024, 1032, 2048, 2056]
SAMPLE_SIZES = [1, 2, 7, 9, 63, 65, 255, 257, 1001]
FMT_IDS = [f.replace("/", "-") for f in sc.FORMATS]

_FIG = {}   # (kernel form, format) -> [launches, buffers, sample positions, largest |error| on the maximum, on the minimum]


def _form(n):
    return "wave" if n % 8 == 0 else "per-sample"


def _dev(raw):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).cuda()


def _run(fmt, n, d_raw, nb, threshold=0.0):
    kind, enob, dc = sc.FORMATS[fmt]
    with Plan(n, FS, threshold, kind=kind, enob=enob, correct_dc=dc, max_batch=nb, mode=capi.MODE_TIME_DOMAIN) as plan:
        plan.submit_device(0, d_raw, nb)
        return plan.collect_time_domain(0)


def _hold(fmt, n, got, want, positions, what):
    """max_db and min_db of a launch against the reference; notes the figures"""
    (mx, mn), (rmx, rmn) = got, want
    print(f"{what}: {len(mx)} buffers; max_db {mx.min()!r} ... {mx.max()!r} (reference {rmx.min()!r} ... {rmx.max()!r}), "
          f"min_db {mn.min()!r} ... {mn.max()!r} (reference {rmn.min()!r} ... {rmn.max()!r})")
    try:
        e_max = sc.agree(mx, rmx, sc.MAX_BAR)
        e_min = sc.agree(mn, rmn, sc.MIN_BAR)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    print(f"{what}: largest |error| {e_max:.2e} dB on the maximum, {e_min:.2e} dB on the minimum")
    f = _FIG.setdefault((_form(n), fmt), [0, 0, 0, 0.0, 0.0])
    f[0], f[1], f[2], f[3], f[4] = f[0] + 1, f[1] + len(mx), f[2] + positions, max(f[3], e_max), max(f[4], e_min)


@pytest.mark.parametrize("n", WAVE_SIZES + SAMPLE_SIZES)
@pytest.mark.parametrize("fmt", sc.FORMATS, ids=FMT_IDS)
def test_every_sample_counts(built_lib, oracle_mod, fmt, n):
    raw, pos_max, pos_min = sc.position(fmt, n)
    rmx, rmn, _ = sc.reference(oracle_mod, fmt, n, raw)
    mx, mn, _ = _run(fmt, n, _dev(raw), len(raw))
    if not sc.FORMATS[fmt][2]:
        # the same values in every buffer, reduced exactly, converted once: no tolerance.  Checked first: a dropped position names itself
        odd_max, odd_min = np.flatnonzero(mx.view(np.uint32) != mx.view(np.uint32)[0]), np.flatnonzero(mn.view(np.uint32) != mn.view(np.uint32)[0])
        assert odd_max.size == 0, f"{fmt} n={n}: max_db differs from buffer 0's ({mx[0]!r}) in buffers {odd_max[:8].tolist()} (maximum at samples {pos_max[odd_max][:8].tolist()}): {mx[odd_max][:8]}"
        assert odd_min.size == 0, f"{fmt} n={n}: min_db differs from buffer 0's ({mn[0]!r}) in buffers {odd_min[:8].tolist()} (minimum at samples {pos_min[odd_min][:8].tolist()}): {mn[odd_min][:8]}"
    _hold(fmt, n, (mx, mn), (rmx, rmn), n, f"{fmt} n={n} position")


def _launch_cases():
    import torch

    grid = 8 * torch.cuda.get_device_properties(0).multi_processor_count   # scn_launch_time_domain: at most 8 blocks per CU
    return grid, [(8, 2 * 4 * grid + 3), (520, 2 * 4 * grid + 3), (9, 2 * grid + 3), (257, 2 * grid + 3), (8, 1), (8, 3), (8, 5)]


def _hold_flags(fmt, n, d_raw, nb, first, what):
    """a second plan whose threshold is the middle LEVEL the first returned: the same values bit for bit, and above == (mx >= thr)"""
    mx, mn, _ = first
    thr = np.float32(sc.middle_threshold(mx))
    mx2, mn2, ab = _run(fmt, n, d_raw, nb, threshold=float(thr))
    assert mx2.tobytes() == mx.tobytes() and mn2.tobytes() == mn.tobytes(), f"{what}: a second launch of the same buffers differs"
    assert np.array_equal(ab, (mx >= thr).astype(np.uint8)), f"{what}: above is not max_db >= {thr!r} (process.cpp:226)"
    assert ab[mx == thr].all() and (mx == thr).any()
    if nb >= 3:
        assert ab.min() == 0 and ab.max() == 1, f"{what}: threshold {thr!r} leaves one outcome only"


@pytest.mark.parametrize("fmt", sc.FORMATS, ids=FMT_IDS)
def test_more_buffers_than_resident_waves(built_lib, oracle_mod, fmt):
    grid, cases = _launch_cases()
    for n, nb in cases:
        raw, _, _ = sc.launch_shape(fmt, n, nb, grid)
        rmx, rmn, _ = sc.reference(oracle_mod, fmt, n, raw)
        d_raw = _dev(raw)
        got = _run(fmt, n, d_raw, nb)
        what = f"{fmt} n={n} launch of {nb} buffers (grid {grid})"
        _hold(fmt, n, got[:2], (rmx, rmn), 0, what)
        _hold_flags(fmt, n, d_raw, nb, got, what)


LONG = [(f, 1 << 20, 3) for f in sc.FORMATS] + [("int8", 1 << 24, 2)]


@pytest.mark.parametrize("fmt,n,nb", LONG, ids=[f"{f.replace('/', '-')}-2^{n.bit_length() - 1}" for f, n, _ in LONG])
def test_long_buffers(built_lib, oracle_mod, fmt, n, nb):
    raw, _, _ = sc.long_buffers(fmt, n, nb)
    rmx, rmn, _ = sc.reference(oracle_mod, fmt, n, raw)
    d_raw = _dev(raw)
    got = _run(fmt, n, d_raw, nb)
    what = f"{fmt} n={n} long"
    _hold(fmt, n, got[:2], (rmx, rmn), 0, what)
    _hold_flags(fmt, n, d_raw, nb, got, what)


@pytest.mark.parametrize("n", [16, 1001])
def test_special_values(built_lib, oracle_mod, n):
    x = sc.special_rows(n)
    o = oracle_mod.Oracle(n)
    ref = [o.time_domain(x[r], threshold=0.0) for r in range(len(x))]
    rmx, rmn = np.array([r[1] for r in ref], np.float32), np.array([r[2] for r in ref], np.float32)
    mx, mn, ab = _run("cfloat", n, _dev(x), len(x))
    for r, name in enumerate(sc.SPECIAL):
        print(f"n={n} {name:<24} max_db {mx[r]!r:>16} (oracle {rmx[r]!r:>16})  min_db {mn[r]!r:>16} (oracle {rmn[r]!r:>16})")
    _hold("cfloat", n, (mx, mn), (rmx, rmn), 0, f"cfloat n={n} special values")
    assert np.array_equal(ab, np.array([r[0] for r in ref], np.uint8))
    plain = sc.SPECIAL.index("plain")          # a NaN or an inf in one buffer leaves the others alone: the rows it cannot reach are the plain row's
    for name in ("NaN in sample 0", "NaN in the last sample"):
        r = sc.SPECIAL.index(name)
        assert (mx[r], mn[r]) == (mx[plain], mn[plain]), name
    for name in ("one +inf", "one power overflows"):
        assert mn[sc.SPECIAL.index(name)] == mn[plain], name


def test_above_flag_on_the_knife_edge(built_lib, oracle_mod):
    n, nb = 8, 6
    raw, _, _ = sc.launch_shape("cfloat", n, nb, 2048)
    raw[5] = 0                                    # an all-zero buffer: the maximum stays the clamp constant
    d_raw = _dev(raw)
    mx, _, ab = _run("cfloat", n, d_raw, nb, threshold=0.0)
    assert mx[5] == np.float32(sc.FLT_MIN) and ab[5] == 1, "numeric_limits<float>::min() >= 0.0: an all-zero buffer is above, as in the reference"
    assert ab.all()
    b = 2
    _, _, at = _run("cfloat", n, d_raw, nb, threshold=float(mx[b]))
    _, _, over = _run("cfloat", n, d_raw, nb, threshold=float(np.nextafter(mx[b], np.float32(np.inf))))
    assert at[b] == 1 and over[b] == 0
    assert np.array_equal(at, (mx >= mx[b]).astype(np.uint8)) and np.array_equal(over, (mx > mx[b]).astype(np.uint8))


def test_zz_figures(request):
    """prints what the module held, per kernel form and format: launches, buffers, sample positions (each the place of the maximum
    of one buffer and of the minimum of another), and the largest |error|; where the whole module ran in this process, asserts that
    every pair was seen"""
    mine = [i for i in request.session.items if i.fspath.basename == "test_time_domain_gpu.py"]
    total = len(sc.FORMATS) * (len(WAVE_SIZES) + len(SAMPLE_SIZES) + 1) + len(LONG) + 2 + 1
    whole = not request.config.option.keyword and not hasattr(request.config, "workerinput") and len(mine) == total + 1
    if whole and mine[-1].name == "test_zz_figures":
        for form in ("wave", "per-sample"):
            for fmt in sc.FORMATS:
                f = _FIG.get((form, fmt))
                assert f and f[0] > 0 and f[1] > 0 and f[2] > 0, (form, fmt, f)
        assert max(f[3] for f in _FIG.values()) <= sc.MAX_BAR and max(f[4] for f in _FIG.values()) <= sc.MIN_BAR
    print(f"build {build.source_hash()}: time-domain mode, {sum(f[0] for f in _FIG.values())} launches")
    print(f"{'kernel form':<12}{'format':<16}{'launches':>8}  {'buffers':>8}  {'positions':>9}  {'max |err| max_db':>16}  {'max |err| min_db':>16}")
    for (form, fmt), f in sorted(_FIG.items()):
        print(f"{form:<12}{fmt:<16}{f[0]:>8}  {f[1]:>8}  {f[2]:>9}  {f[3]:>16.2e}  {f[4]:>16.2e}")
