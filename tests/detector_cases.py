"""The case matrix of tests/test_detector_geometry_gpu.py, stated once: which instantiation of its kernel a size reaches in each of
the three detectors behind the transform, the masks, the windows and the sizes.  tests/test_detector_cases_cpu.py holds the three
`*_instance` functions to the launchers' own lines (as tests/test_launch_caps_cpu.py holds tests/launch_caps.py), so that a moved
step fails on a CPU instead of silently taking a GPU case off the instantiation it was chosen for.

  detector            launcher (file)                                    instantiation
  floor window        scn_launch_floor_local (scn_floor_local.hip)       <T, RUNS>: a tile is 4 T RUNS fftshift indices
  unit-wide floor     scn_launch_floor (scn_floor.hip)                   <T, KPT, REREAD>: KPT bins per thread in registers, or re-read
  baseline            scn_launch_baseline_detect (scn_baseline.hip)      <T, VEC, U>: 16-byte or 4-byte loads, U loads in flight
"""

# ---- scn_floor_local.hip, scn_launch_floor_local --------------------------------------------------------------------------------
LOCAL_FLOOR_STEPS = [(256, (64, 1)), (512, (64, 2)), (1024, (256, 1)), (4096, (256, 4)), (8192, (1024, 2))]
LOCAL_FLOOR_LAST = (1024, 4)


def local_floor_instance(n):
    """(T, RUNS) of scn_floor_local_kernel at n points"""
    for top, inst in LOCAL_FLOOR_STEPS:
        if n <= top:
            return inst
    return LOCAL_FLOOR_LAST


def local_floor_tiles(n):
    """(tiles, bins of the last tile): `for (uint32_t tile0 = 0; tile0 < n; tile0 += G::CAP)`, CAP = 4 T RUNS"""
    t, runs = local_floor_instance(n)
    cap = 4 * t * runs
    tiles = -(-n // cap)
    return tiles, n - (tiles - 1) * cap


# ---- scn_floor.hip, scn_launch_floor --------------------------------------------------------------------------------------------
FLOOR_STEPS = [(128, (64, 2, False)), (512, (64, 8, False)), (1024, (256, 4, False)), (4096, (256, 16, False)), (8192, (1024, 8, False)),
               (16384, (1024, 16, False))]
FLOOR_LAST = (1024, 1, True)


def floor_instance(n):
    """(T, KPT, REREAD) of scn_floor_kernel at n points"""
    for top, inst in FLOOR_STEPS:
        if n <= top:
            return inst
    return FLOOR_LAST


def floor_reread_trips(n):
    """(trips of the re-read route, threads of the last trip that hold a bin): `trips = REREAD ? (n + T - 1u) / T`"""
    t, _, reread = floor_instance(n)
    assert reread
    trips = -(-n // t)
    return trips, n - (trips - 1) * t


# ---- scn_baseline.hip, scn_launch_baseline_detect -> launch_size -> launch_team -------------------------------------------------
BASELINE_TEAM_STEPS = [(512, 64), (4096, 256)]  # launch_size: `if (a.n <= 512u)`, `if (a.n <= 4096u)`
BASELINE_TEAM_LAST = 1024


def baseline_instance(n, aligned=True):
    """(T, VEC, U) of scn_baseline_kernel at n points; aligned: both base pointers are 16-byte aligned (device allocations are)"""
    vec = n % 4 == 0 and aligned
    t = BASELINE_TEAM_LAST
    for top, team in BASELINE_TEAM_STEPS:
        if n <= top:
            t = team
            break
    per_trip = t * (4 if vec else 1)
    trips = -(-n // per_trip)
    return t, vec, 1 if trips <= 1 else 2 if trips <= 2 else 4


def baseline_loop_trips(n, aligned=True):
    """iterations of `for (uint32_t k0 = 0; k0 < trips; k0 += (uint32_t)U)`"""
    t, vec, u = baseline_instance(n, aligned)
    trips = -(-n // (t * (4 if vec else 1)))
    return -(-trips // u)


N_MIN, N_MAX = 16, 65536  # the sizes a plan takes


def reachable(instance, **kw):
    """every instantiation some size of a plan reaches"""
    return {instance(n, **kw) for n in range(N_MIN, N_MAX + 1)}


# ---- the matrix -----------------------------------------------------------------------------------------------------------------
MASKS = [(0.75, 4), (1.0, 0), (0.5, 8), (0.9, 1), (1.0, 4)]  # (use_bandwidth, dc_ignore_bins)
DEFAULT_MASK, FULL_MASK = MASKS[0], MASKS[1]
OTHER_MASKS = MASKS[1:]

# (train, guard): every small window -- each guard mod 4 with guard <= 2 and above, each train mod 4 -- and twelve at or near the limits
SWEEP = [(train, guard) for train in range(1, 13) for guard in range(10)] + [
    (127, 63), (128, 61), (125, 64), (37, 11), (64, 0), (3, 64), (128, 0), (1, 64), (128, 64), (2, 63), (126, 62), (5, 33)]
SWEEP_SIZES = [256, 1024]
# the windows of SWEEP that leave an evaluated bin without a cell: {(n, mask): windows}; every other one is valid
SWEEP_INVALID = {(256, DEFAULT_MASK): [(3, 64), (1, 64), (2, 63)], (256, FULL_MASK): [], (1024, DEFAULT_MASK): [], (1024, FULL_MASK): []}

# one window per pair (guard mod 4, train mod 4), then six at or near the limits (which also run at the lowest and the highest rank)
RESIDUES = [(12, 0), (21, 4), (6, 8), (35, 16), (40, 5), (1, 9), (14, 1), (27, 13), (64, 2), (9, 6), (2, 10), (19, 30), (8, 3), (33, 7),
            (10, 11), (3, 3)] + [(128, 64), (127, 63), (128, 0), (1, 0), (125, 62), (126, 61)]
RESIDUES_EXTRA = RESIDUES[16:]
RESIDUE_SIZES = [301, 512, 4096, 8192, 16384, 20000, 32768, 65535]

EDGE_SIZES = [90, 301, 501, 2048, 3000, 4097, 10000, 20000, 32768, 65535]  # under the default mask
# under every other mask.  512 is here for the baseline's <64, VEC, 2>: 260 ... 512 points in steps of 4, which no other list holds
MASK_SIZES = [16, 64, 512, 1001, 4096, 8192, 65536]
# 4097 once more with the DC hole closed: the fifth trip of the baseline's <1024, scalar, 4> and the floor's ninth bin per thread hold
# ONE bin, natural bin 4096, which the default mask removes -- under it nothing that trip does can show
EXTRA_UNIT_CASES = [(4097, FULL_MASK)]

AVERAGE_SIZES = [1024, 2048, 4096, 8192]
AVERAGE_ROUTES = [(3, 2, False), (1, 16, True)]  # (groups, K, split: several workgroups share a group)
AVERAGE_MASKS = [(1.0, 0), (0.5, 8), (0.9, 1)]
AVERAGE_DETECTOR_SIZES = {"floor": 2048, "window": 4096, "baseline": 1024}  # one averaged case each, under the full mask

SIGNAL_SIZES = [64, 1001, 4096, 65535, 65536]


def units_for(n):
    """units of a geometry case: 2 to 5, fewer where a unit is large"""
    return 5 if n <= 1024 else 3 if n <= 8192 else 2
