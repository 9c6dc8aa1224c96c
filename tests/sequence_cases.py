"""Whole plan sequences, drawn from a seed: what tests/test_plan_sequences_gpu.py runs on the GPU and tests/test_sequence_cases_cpu.py
holds to its coverage conditions on the CPU.  Pure Python and numpy: no GPU, no library.

draw(seed) returns SCRIPTS_PER_SEED plan scripts.  A script is {"plan": a plan description, "steps": [step, ...]}, made of Python
literals only, so that repr(script) can be pasted into a regression test.  A step names its input by the seed of its scene, never by
samples (scene() makes them), and carries the status it must return: OK, or the refusal it is there for.

The generator keeps a small state of its own (pending slots, table, window, baseline rows) so that every step it draws is legal
under include/scanner_hip.h; tests/sequence_model.py restates those rules independently and the CPU test holds the two together.
"""
import numpy as np

from scanner_amd import capi
from tests import detector_cases, local_floor_ref
from tests import tolerances as tol

FS = 8000000
SCRIPTS_PER_SEED = 4
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS

# the size families: (what the size is there for, the sizes)
FAMILIES = {
    "small": [16, 64],          # one bitmap word, the small multi-buffer kernels
    "wave": [512],              # the largest wave-per-unit detector size
    "mixed": [1000, 12000],     # both mixed-radix forms
    "bluestein": [1001],
    "averaged": [1024, 2048, 4096, 8192],  # every averaged size; 8192: the largest fused size of the averaged kernels
    "fused-top": [16384],       # the largest fused size
    "four-step": [32768, 65536],  # the four-step pair; the four-tile window detector and the floor route that re-reads
}
FAMILY_OF = {n: f for f, sizes in FAMILIES.items() for n in sizes}
SIZES = sorted(FAMILY_OF)
DETECTORS = ("fixed", "floor", "window", "baseline")
KINDS = (capi.KIND_BYTE_COMPLEX, capi.KIND_SHORT, capi.KIND_SHORT_COMPLEX, capi.KIND_FLOAT_COMPLEX)
PERMILLES = (0, capi.FLOOR_MIN, 1, 250, 999, 1000)
AVERAGES = (1, 2, 3, 4, 8, 64)
SPECIALS = ("zero", "const", "nan", "overflow")
REFUSALS = ("state_pending", "bad_nb", "rows_mismatch", "collect_idle")
OVERFLOW_AMPLITUDE = 2.0 ** 68  # its transform's peak exceeds 2^64 under every window: the bin's power is +inf, far bins stay finite

# The committed seed list: chosen by search_seeds() until tests/test_sequence_cases_cpu.py's coverage conditions hold
SEEDS = (2414, 2240, 488, 119, 386, 237, 362, 280, 49)


def max_units(n):
    """units per submit at the most: the smallest shapes with a second unit per team, a second slot, a ragged last workgroup"""
    return 48 if n <= 1024 else 12 if n <= 8192 else 3


def members(g, groups, k, layout):
    """the buffers of group g in a submit of groups * k buffers"""
    return g + groups * np.arange(k) if layout == capi.AVG_SWEEPS else g * k + np.arange(k)


def quant(plan):
    """(LSB per unit of the float scene, the dB level the scene's noise median lands on) of the plan's wire format"""
    if plan["kind"] == capi.KIND_FLOAT_COMPLEX:
        return 1.0, 0.0
    lsb = 8.0 if plan["kind"] == capi.KIND_BYTE_COMPLEX else 100.0  # the noise's sigma in LSB
    q = lsb * np.sqrt(plan["n"]) / 1.67
    return q, 10.0 * np.log10(q / 2.0 ** (plan["enob"] - 1))


def scene(plan, seed, units, specials=None):
    """The raw buffers of one submit (or of a baseline's rows), in the plan's wire format: [units * K, ...].  Noise straddling 0 dB
    (tests/test_floor_gpu.py, _straddling) with a gain and a tone per unit, so that a unit taken for another moves whole dB; every
    buffer of an averaged group shares its unit's gain and tone.  specials: {unit: (kind, argument)} replaces whole units."""
    n, k, layout, kind = plan["n"], plan["average"], plan["layout"], plan["kind"]
    nb = units * k
    rng = np.random.default_rng([int(seed), 77])
    x = (rng.standard_normal((nb, n, 2), dtype=np.float32) * np.float32(1.67 / np.sqrt(n))).view(np.complex64).reshape(nb, n)
    t = np.arange(n)
    gains = rng.uniform(0.4, 1.0, units)
    offset = int(rng.integers(1, 20))
    for u in range(units):
        j = 1 + (97 * u + 13 + int(seed)) % (n // 2 - 1)
        tone = ((10.0 / (0.36 * n)) * np.exp(2j * np.pi * (j + 0.25) * t / n)).astype(np.complex64)
        for b in members(u, units, k, layout):
            x[b] = (x[b] + tone) * np.float32(gains[u])
    if kind == capi.KIND_FLOAT_COMPLEX:
        raw = x
    else:
        q, _ = quant(plan)
        top = 127 if kind == capi.KIND_BYTE_COMPLEX else 32767
        v = np.rint(x.view(np.float32).reshape(nb, n, 2) * np.float32(q)).astype(np.int64)
        if plan["correct_dc"]:  # a positive mean (the negative-sum quirk of the reference has a test of its own)
            v += offset if kind == capi.KIND_BYTE_COMPLEX else 15 * offset
        raw = np.clip(v, -top, top).astype(np.int8 if kind == capi.KIND_BYTE_COMPLEX else np.int16)
        if kind == capi.KIND_SHORT:  # planar: I[n] then Q[n]
            raw = np.ascontiguousarray(raw.transpose(0, 2, 1))
    for u, (what, arg) in (specials or {}).items():
        for b in members(int(u), units, k, layout):
            if what == "zero":
                raw[b] = 0
            elif what == "const":
                raw[b] = arg
            elif what == "nan":
                raw[b, arg] = np.nan
            else:
                assert what == "overflow"
                raw[b] = ((OVERFLOW_AMPLITUDE / n) * np.exp(2j * np.pi * arg * t / n)).astype(np.complex64)
    return raw


def headers(plan, step):
    """(center_freqs per buffer | None, seq_ids per buffer | None) of a submit step, as the caller passes them"""
    units, k, layout = step["units"], plan["average"], plan["layout"]
    nb = step["nb"]
    fc = seq = None
    if not step["indexed"]:
        fc = np.zeros(nb)
        if nb % k == 0:
            for g in range(units):
                fc[members(g, units, k, layout)] = step["fc0"] + 6e6 * g
    if step["seq0"] is not None:
        seq = np.uint64(step["seq0"]) + np.uint64(3) * np.arange(nb, dtype=np.uint64)
    return fc, seq


def table_of(step):
    return step["base"] + 6e6 * ((7 * np.arange(step["count"])) % max(1, step["count"]))


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _evaluated(n, mask):
    return np.flatnonzero(tol.evaluated_mask(n, *mask))


def _draw_plan(rng):
    family = str(rng.choice(list(FAMILIES)))
    n = int(rng.choice(FAMILIES[family]))
    detect = str(rng.choice(DETECTORS))
    kind = int(rng.choice(KINDS))
    enob = 8 if kind == capi.KIND_BYTE_COMPLEX else 12 if kind == capi.KIND_FLOAT_COMPLEX else int(rng.choice([10, 12, 14]))
    while True:
        mask = detector_cases.MASKS[int(rng.integers(len(detector_cases.MASKS)))]
        if _evaluated(n, mask).size:
            break
    k = int(rng.choice(AVERAGES)) if family == "averaged" and rng.random() < 0.7 else 1
    top = max_units(n)
    if k == 64:
        top = 3 if n <= 2048 else 2
    units = int(rng.integers(min(2, top), top + 1))
    if k > 1 and rng.random() < 0.5:
        units = min(units, 3)
    if detect == "fixed":
        flags = int(rng.choice([BOTH, BOTH, capi.OUT_HITS, capi.OUT_HITS, capi.OUT_SPECTRUM]))
    else:
        flags = int(rng.choice([BOTH, capi.OUT_HITS]))
    plan = dict(n=n, kind=kind, enob=enob, correct_dc=bool(rng.integers(2)) and kind != capi.KIND_FLOAT_COMPLEX,
                use_bandwidth=float(mask[0]), dc_ignore_bins=int(mask[1]), trigger_count=int(rng.choice([0, max(1, n // 8), 1047])),
                max_batch=units * k, max_hits=int(rng.choice([4, 16, 100])) if rng.random() < 0.35 else 0, flags=flags,
                overlap=bool(rng.integers(2)), detect=detect, permille=int(rng.choice(PERMILLES)) if detect in ("floor", "window") else 0,
                average=k, layout=int(rng.choice([capi.AVG_DWELL, capi.AVG_SWEEPS])) if k > 1 else capi.AVG_DWELL, threshold=0.0)
    if detect == "fixed":  # about the noise's own level: a good share of the evaluated bins on either side
        plan["threshold"] = float(np.float32(quant(plan)[1] - 2.0 + float(rng.choice([-1.0, 0.0, 2.0]))))
    else:
        plan["threshold"] = float(rng.choice([0.0, 1.0, 3.0]))
    return plan


def _windows(plan, rng, count):
    """`count` distinct valid windows from tests/detector_cases.py's sweep (small trains only where a unit is large: the numpy
    reference sorts a row of 2 * train cells per evaluated bin)"""
    n, mask = plan["n"], (plan["use_bandwidth"], plan["dc_ignore_bins"])
    out = []
    for w in rng.permutation(len(detector_cases.SWEEP)):
        train, guard = detector_cases.SWEEP[int(w)]
        if n > 8192 and train > 12:
            continue
        if local_floor_ref.valid(n, train, guard, *mask):
            out.append((int(train), int(guard)))
            if len(out) == count:
                break
    return out


class _Gen:
    """one script: the plan, the steps so far and the generator's own view of the plan's state"""

    def __init__(self, rng):
        self.rng = rng
        self.plan = _draw_plan(rng)
        self.steps = []
        self.pending = []            # slots, in submit order
        self.units = {}              # slot: units of its last accepted submit
        self.collected = set()       # slots submitted and collected (update_baseline's condition)
        self.table = 0
        self.rows = 0
        self.window = (0, 0)
        self.top = self.plan["max_batch"] // self.plan["average"]
        self.has_hits = bool(self.plan["flags"] & capi.OUT_HITS)
        self.windows = _windows(self.plan, rng, 3) if self.plan["detect"] == "window" else []
        self.refusal = str(rng.choice(REFUSALS)) if rng.random() < 0.4 else None

    def add(self, op, expect=capi.OK, **kw):
        self.steps.append(dict(op=op, expect=int(expect), **kw))

    # -- state changes (no slot pending) --
    def set_table(self, count=None):
        choices = [c for c in (1, 2, self.top, self.top + 3, 2 * self.top + 1) if c != self.table]
        count = int(self.rng.choice(choices)) if count is None else count
        self.add("set_table", count=count, base=float(50e6 + int(self.rng.integers(0, 1000))))
        self.table = count

    def set_window(self, window):
        self.add("set_window", train=window[0], guard=window[1])
        self.window = window

    def set_baseline(self, rows=None, learn=None):
        if rows is None:
            choices = [r for r in {1, self.top, self.top + 2, self.table or 2} if r != self.rows]
            rows = int(self.rng.choice(sorted(choices)))
        learn = (self.rng.random() < 0.35) if learn is None else learn
        self.add("set_baseline", rows=rows, seed=None if learn else int(self.rng.integers(1 << 30)))
        self.rows = rows

    def state_changes(self):
        rng, detect = self.rng, self.plan["detect"]
        if rng.random() < 0.5:
            self.set_table()
        if detect == "window" and rng.random() < 0.8:
            others = [w for w in self.windows + [(0, 0)] if w != self.window]
            self.set_window(others[int(rng.integers(len(others)))])
        if detect == "baseline":
            for slot in rng.permutation(sorted(self.collected)):
                if self.rows and self.units[int(slot)] <= self.rows and rng.random() < 0.7:
                    self.add("update_baseline", slot=int(slot), mode=int(rng.choice([capi.BASELINE_SET, capi.BASELINE_MAX])))
            if rng.random() < 0.5:
                self.add("get_baseline")
            if rng.random() < 0.4:
                self.set_baseline()

    # -- submits and collects --
    def indexed_ok(self):
        return self.table > 0 and (self.plan["detect"] != "baseline" or self.rows in (1, self.table))

    def submit(self, slot, units=None):
        rng, k = self.rng, self.plan["average"]
        if units is None:
            units = int(rng.choice([0, 1, int(rng.integers(0, self.top + 1)), self.top, self.top]))
        indexed = self.has_hits and self.indexed_ok() and rng.random() < 0.5
        first = int(rng.integers(0, self.table)) if indexed else 0
        if indexed and self.table > 1 and rng.random() < 0.5:
            first = max(first, self.table - 1 - int(rng.integers(0, 2)))  # a run that wraps
        specials = {}
        evaluated = _evaluated(self.plan["n"], (self.plan["use_bandwidth"], self.plan["dc_ignore_bins"]))
        for u in range(1, units - 1):  # between ordinary units
            if rng.random() < 0.125 * (3 if units <= 3 else 1) and (u - 1) not in specials:
                what = str(rng.choice(SPECIALS if self.plan["kind"] == capi.KIND_FLOAT_COMPLEX else SPECIALS[:2]))
                arg = {"zero": 0, "const": int(rng.integers(1, 9)), "nan": int(rng.integers(self.plan["n"])),
                       "overflow": int(evaluated[int(rng.integers(evaluated.size))])}[what]
                specials[u] = (what, arg)
        self.add("submit", slot=slot, units=units, nb=units * k, pinned=bool(rng.random() < 0.4), indexed=indexed, first_index=first,
                 fc0=float(100e6 + int(rng.integers(0, 1000))), seq0=int(rng.integers(0, 1 << 40)) if rng.random() < 0.5 else None,
                 seed=int(rng.integers(1 << 30)), specials=specials)
        self.pending.append(slot)
        self.units[slot] = units

    def post_ops(self):
        rng, n = self.rng, self.plan["n"]
        ops = []
        if not self.has_hits:
            return ops
        for _ in range(int(rng.integers(0, 3))):
            ops.append(("more", float(rng.choice([0.0, 0.3, 0.7, 1.0])), float(rng.choice([0.1, 0.5, 1.5]))))
        for _ in range(int(rng.integers(0, 3))):  # (gap, first and cap as shares of the total: inside a unit; 1.1: past the end)
            ops.append(("signals", int(rng.choice([0, 1, 7, 31, 32, n])), float(rng.choice([0.0, 0.37, 0.61, 1.1])), float(rng.choice([0.21, 0.5, 1.0]))))
        if self.plan["detect"] in ("floor", "window") and rng.random() < 0.7:
            ops.append(("floor",))
        if rng.random() < 0.5:
            ops.append(("view",))
        return [ops[int(i)] for i in rng.permutation(len(ops))]

    def collect(self, slot):
        self.pending.remove(slot)
        self.collected.add(slot)
        self.add("counts" if self.rng.random() < 0.2 else "collect", slot=slot, post=self.post_ops())

    # -- refusals: each carries its status, and the sequence goes on --
    def refuse_state_pending(self):
        detect = self.plan["detect"]
        kinds = ["set_table"] + (["set_window"] if detect in ("floor", "window") else []) + (["set_baseline", "update_baseline"] if detect == "baseline" else [])
        what = str(self.rng.choice(kinds))
        if what == "set_table":
            self.add("set_table", capi.E_STATE, count=self.table + 1, base=float(51e6))
        elif what == "set_window":
            w = next((w for w in (self.windows or _windows(self.plan, self.rng, 1)) if w != self.window), (0, 0))
            self.add("set_window", capi.E_STATE, train=w[0], guard=w[1])
        elif what == "set_baseline":
            self.add("set_baseline", capi.E_STATE, rows=self.rows + 1, seed=int(self.rng.integers(1 << 30)))
        else:
            self.add("update_baseline", capi.E_STATE, slot=int(self.rng.integers(capi.NUM_SLOTS)), mode=capi.BASELINE_SET)

    def refuse_bad_nb(self, slot):
        k = self.plan["average"]
        nb = self.plan["max_batch"] + k if (k == 1 or self.rng.random() < 0.5) else self.plan["max_batch"] - 1
        self.add("submit", capi.E_INVALID, slot=slot, units=nb // k, nb=nb, pinned=False, indexed=False, first_index=0, fc0=100e6, seq0=None,
                 seed=int(self.rng.integers(1 << 30)), specials={})

    def refuse_rows_mismatch(self, slot):
        """a baseline whose row count is neither 1 nor the table's, then an indexed submit"""
        if not self.table:
            self.set_table()
        self.set_baseline(rows=self.table + 1 + (self.table == 0), learn=False)
        self.add("submit", capi.E_STATE, slot=slot, units=1, nb=self.plan["average"], pinned=False, indexed=True, first_index=0, fc0=100e6,
                 seq0=None, seed=int(self.rng.integers(1 << 30)), specials={})

    def run(self):
        rng, detect = self.rng, self.plan["detect"]
        if rng.random() < 0.7 or detect == "baseline":
            self.set_table()
        if detect == "window":
            self.set_window(self.windows[0])
        if detect == "baseline":
            self.set_baseline(rows=int(rng.choice([1, self.table, self.top, self.top + 2])))
        refusal, rounds = self.refusal, int(rng.integers(2, 4))
        at = int(rng.integers(rounds))
        for r in range(rounds):
            slots = [int(s) for s in rng.permutation(capi.NUM_SLOTS)[:int(rng.choice([1, 2, 3, 4]))]]
            for slot in slots:
                units = None
                if slot in self.units and self.units[slot] > 1 and rng.random() < 0.5:
                    units = int(rng.integers(1, self.units[slot]))  # fewer units than this slot's last submit
                self.submit(slot, units)
            if refusal == "state_pending" and r == at:
                self.refuse_state_pending()
            if refusal == "bad_nb" and r == at:
                self.refuse_bad_nb(next((s for s in range(capi.NUM_SLOTS) if s not in self.pending), self.pending[0]))
            order = [int(s) for s in rng.permutation(self.pending)]
            for slot in order:
                self.collect(slot)
            if refusal == "collect_idle" and r == at:
                self.add("collect", capi.E_STATE, slot=int(rng.integers(capi.NUM_SLOTS)), post=[])
            if refusal == "rows_mismatch" and r == at and detect == "baseline" and self.has_hits:
                self.refuse_rows_mismatch(int(rng.integers(capi.NUM_SLOTS)))
            if r + 1 < rounds:
                self.state_changes()
        if detect == "baseline":
            self.add("get_baseline")
        return dict(plan=self.plan, steps=self.steps)


def draw(seed):
    """the plan scripts of one seed"""
    return [_Gen(np.random.default_rng([int(seed), index])).run() for index in range(SCRIPTS_PER_SEED)]


# ---- what a list of scripts covers (tests/test_sequence_cases_cpu.py's conditions; search_seeds() below) -------------------------
def allowed_pairs():
    """every (detector, size family) pair the header allows: each detector runs at every size"""
    return {(d, f) for d in DETECTORS for f in FAMILIES}


def coverage(scripts):
    """the set of things the scripts cover, as hashable labels"""
    got = set()
    for sc in scripts:
        plan, steps = sc["plan"], sc["steps"]
        k = plan["average"]
        got.add(("pair", plan["detect"], FAMILY_OF[plan["n"]]))
        got.add(("size", plan["n"]))
        got.add(("kind", plan["kind"]))
        got.add(("flags", plan["detect"], plan["flags"]))
        got.add(("overlap", plan["overlap"]))
        if plan["max_hits"]:
            got.add(("small max_hits",))
        if k > 1:
            got.add(("layout", plan["layout"]))
            got.add(("parts", "one" if k <= 2 else "many"))  # scn_plan_average_parts: at most (K + 1) / 2 parts when the groups are few
            got.add(("average", k))
        pending, units, window, table, rows = [], {}, (0, 0), 0, 0
        nan_held = False  # a max-hold of a NaN unit that no later SET or set_baseline has overwritten
        learnt, submitted, nan_units = False, set(), set()  # the baseline holds finite rows; slots with something to fold; slots whose last submit has a NaN unit
        for st in steps:
            op, ok = st["op"], st["expect"] == capi.OK
            if not ok:
                if op == "submit":
                    got.add(("refusal", "rows_mismatch" if st["indexed"] else "bad_nb"))
                elif op == "collect":
                    got.add(("refusal", "collect_idle"))
                else:
                    got.add(("refusal", "state_pending"))
                    got.add(("refusal", "state_pending", op))
                continue
            got.add(("op", op))
            if op == "submit":
                got.add(("submit", "pinned" if st["pinned"] else "device"))
                got.add(("submit", "indexed" if st["indexed"] else "centres"))
                got.add(("submit", "seq" if st["seq0"] is not None else "no seq"))
                if st["indexed"] and st["first_index"] + st["units"] > table:
                    got.add(("submit", "wraps"))
                if st["indexed"] and k > 1 and any(g * (k - 1) % table for g in range(st["units"])):
                    got.add(("submit", "averaged indexed"))  # (a group whose entry differs from the one its first BUFFER's index names)
                if plan["detect"] == "baseline" and st["indexed"] and st["units"] and learnt and st["first_index"] % rows:
                    got.add(("baseline", "rows from first_index"))
                submitted.add(st["slot"])
                (nan_units.add if any(w == "nan" for w, _ in st["specials"].values()) else nan_units.discard)(st["slot"])
                if st["nb"] == 0:
                    got.add(("submit", "nb == 0"))
                if st["units"] == plan["max_batch"] // k:
                    got.add(("submit", "max_batch"))
                if st["slot"] in units and st["units"] < units[st["slot"]]:
                    got.add(("submit", "fewer units than before"))
                for what, _ in st["specials"].values():
                    got.add(("special", what))
                pending.append(st["slot"])
                units[st["slot"]] = st["units"]
                if len(pending) >= 3:
                    got.add(("three slots in flight",))
            elif op in ("collect", "counts"):
                if pending and pending[0] != st["slot"]:
                    got.add(("collect order differs",))
                pending.remove(st["slot"])
                for p in st["post"]:
                    got.add(("post", p[0]))
                    if p[0] == "signals":
                        got.add(("gap", "n" if p[1] == plan["n"] else p[1]))
                        if p[2] > 1.0:
                            got.add(("signals", "past the end"))
            elif op == "set_table":
                if table:
                    got.add(("table", "larger" if st["count"] > table else "smaller"))
                table = st["count"]
            elif op == "set_window":
                new = (st["train"], st["guard"])
                if window != (0, 0) and new != (0, 0):
                    got.add(("window", "changed"))
                    if new[0] == window[0] and new[1] != window[1]:
                        got.add(("window", "guard alone changed"))
                if window != (0, 0) and new == (0, 0):
                    got.add(("window", "back to none"))
                if window == (0, 0) and new != (0, 0) and ("window", "back to none") in got:
                    got.add(("window", "set again"))
                window = new
            elif op == "set_baseline":
                if rows and st["rows"] != rows:
                    got.add(("baseline", "re-sized"))
                if st["seed"] is None:
                    got.add(("baseline", "rows of +inf"))
                rows, learnt, nan_held = st["rows"], st["seed"] is not None, False
            elif op == "update_baseline":
                got.add(("update", "SET" if st["mode"] == capi.BASELINE_SET else "MAX"))
                if units[st["slot"]]:
                    learnt = True
                if st["slot"] > min(submitted):
                    got.add(("update", "not the lowest slot"))
                if st["mode"] == capi.BASELINE_SET:
                    nan_held = False
                elif st["slot"] in nan_units and learnt:
                    nan_held = True
            elif op == "get_baseline" and nan_held:
                got.add(("update", "MAX of a NaN unit, read back"))
    return got


def required():
    """what the committed seed list must cover"""
    need = {("pair", d, f) for d, f in allowed_pairs()}
    need |= {("size", n) for n in SIZES} | {("kind", k) for k in KINDS}
    need |= {("layout", capi.AVG_DWELL), ("layout", capi.AVG_SWEEPS), ("parts", "one"), ("parts", "many")}
    need |= {("average", k) for k in AVERAGES if k > 1}
    need |= {("op", o) for o in ("submit", "collect", "counts", "set_table", "set_window", "set_baseline", "update_baseline", "get_baseline")}
    need |= {("post", p) for p in ("more", "signals", "floor", "view")}
    need |= {("refusal", r) for r in REFUSALS}
    need |= {("refusal", "state_pending", o) for o in ("set_table", "set_window", "set_baseline", "update_baseline")}
    need |= {("submit", s) for s in ("pinned", "device", "indexed", "centres", "seq", "no seq", "wraps", "averaged indexed", "nb == 0", "max_batch",
                                     "fewer units than before")}
    need |= {("special", s) for s in SPECIALS}
    need |= {("gap", g) for g in (0, 1, 7, 31, 32, "n")} | {("signals", "past the end")}
    need |= {("window", "changed"), ("window", "guard alone changed"), ("window", "back to none"), ("table", "larger"), ("table", "smaller"), ("baseline", "re-sized"),
             ("baseline", "rows of +inf"), ("baseline", "rows from first_index"), ("update", "SET"), ("update", "MAX"),
             ("update", "not the lowest slot"), ("update", "MAX of a NaN unit, read back"), ("three slots in flight",), ("collect order differs",),
             ("small max_hits",), ("overlap", True), ("overlap", False)}
    need |= {("flags", d, f) for d in DETECTORS for f in (BOTH, capi.OUT_HITS)} | {("flags", "fixed", capi.OUT_SPECTRUM)}
    return need


def search_seeds(candidates=range(4000), cost=None):
    """a greedy cover of required() by seeds (how SEEDS was chosen): repeatedly the seed that covers most of what is still missing"""
    need, chosen = required(), []
    covers = {s: coverage(draw(s)) & need for s in candidates}
    while need:
        best = max(covers, key=lambda s: (len(covers[s] & need), -s))
        if not covers[best] & need:
            raise AssertionError(f"no candidate covers {sorted(need, key=str)}")
        chosen.append(best)
        need -= covers[best]
    return chosen
