"""Whole plan sequences, drawn from a seed: what tests/test_plan_sequences_gpu.py runs on the GPU and tests/test_sequence_cases_cpu.py
holds to its coverage conditions on the CPU.  Pure Python and numpy: no GPU, no library.

draw(seed) returns SCRIPTS_PER_SEED plan scripts.  A script is {"plan": a plan description, "steps": [step, ...]}, made of Python
literals only, so that repr(script) can be pasted into a regression test.  A step names its input by the seed of its scene, never by
samples (scene() makes them), and carries the status it must return: OK, or the refusal it is there for.

The generator keeps a small state of its own (pending slots, table, window, baseline rows) so that every step it draws is legal
under include/scanner_hip.h; tests/sequence_model.py restates those rules independently and the CPU test holds the two together.

The steps of the hit history, the sweep trace, the level histogram and the trace emitters (NEW_OPS) are drawn in a second pass, from
a random stream of their own, and laid between the steps of the first: they change nothing a step of the first pass depends on, and
strip_new(script) gives the script of the first pass back exactly (tests/test_sequence_cases_cpu.py pins its sha256 per seed).
"""
import numpy as np

from scanner_amd import capi
from tests import detector_cases, emitters_ref, local_floor_ref, trace_ref
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
SEEDS = (2414, 2240, 488, 119, 386, 237, 362, 280, 49, 10)

# the second pass: the hit history, the sweep trace, the level histogram, the trace emitters
NEW_OPS = ("set_history", "update_history", "get_history", "confirmed", "set_trace", "update_trace", "get_trace", "merge_trace", "emitters",
           "set_levels", "update_levels", "get_levels", "levels_summary")
MAX_NEW_STEPS = 45  # per script
CONFIRMS = ((1, 1), (1, 2), (2, 2), (2, 3), (3, 4), (1, 32), (32, 32))  # (m, window)
CELL_COUNTS = (1, 37, 200, 1023, 1024, 1025, 1300)  # the emitters' kernels work a wave per 1024 cells; 1300: a run can cross the seam
LEVEL_CELLS = (1, 8, 37, 200)
EDGE_KINDS = ("one", "few", "many")
GAPS = (0, 1, 7, "cells")
LINES = (capi.TRACE_LINE_MAX, capi.TRACE_LINE_MIN, capi.TRACE_LINE_SPREAD)


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


def edges_of(plan, kind):
    """the level table of a set_levels step: one edge at the scene's noise level, a few straddling it, or all 255"""
    q = quant(plan)[1]
    e = [q] if kind == "one" else [q - 3.0, q - 0.5, q + 0.5, q + 3.0, q + 8.0] if kind == "few" else q - 40.0 + 60.0 * np.arange(255) / 254.0
    return np.asarray(e, np.float32)


def merge_window(step):
    """the host window of a merge_trace step: emitters_ref.seeded_trace, with empty cells; nan: a NaN in max_db (even) or min_db (odd)"""
    max_db, min_db, count = emitters_ref.seeded_trace(step["cells"], step["seed"], 0.3)
    if step["nan"] is not None:
        (max_db, min_db)[step["nan"] % 2][(step["nan"] // 2) % step["cells"]] = np.nan
    return max_db, min_db, count


def emitter_threshold(plan, step):
    """about the scene's noise level, or about its tone level (max and min lines); a spread of a few dB"""
    return float(np.float32(step["level"] + (0.0 if step["line"] == capi.TRACE_LINE_SPREAD else quant(plan)[1])))


def unit_centres(plan, step, table):
    """the centre of every unit of an accepted submit: its own, or the run of the table (a set_table step) it names"""
    if step["indexed"]:
        fc = table_of(table)
        return fc[(step["first_index"] + np.arange(step["units"])) % fc.size]
    return step["fc0"] + 6e6 * np.arange(step["units"])


def strip_new(script):
    """the script of the first pass: without the steps of NEW_OPS and the caller's-buffer mark of a submit"""
    return dict(plan=script["plan"], steps=[{k: v for k, v in st.items() if k != "out"} for st in script["steps"] if st["op"] not in NEW_OPS])


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


# ---- the second pass ---------------------------------------------------------------------------------------------------------------
class Track:
    """What a script's steps so far have left behind, as far as the steps of NEW_OPS depend on it: fed every step in order, it says
    which status such a step must carry (status) and why (reason), and keeps which cells of the trace are occupied, by which slots.
    The second pass labels its steps with it and coverage() reads its conditions from it."""

    def __init__(self, plan):
        self.plan = plan
        self.has_hits = bool(plan["flags"] & capi.OUT_HITS)
        self.can_trace = self.has_hits and (bool(plan["flags"] & capi.OUT_SPECTRUM) or plan["detect"] != "fixed")
        self.pending, self.sub, self.last, self.before, self.listed = [], {}, {}, {}, set()
        self.table = None
        self.rows, self.epoch, self.folded, self.set_history_since = 0, 0, {}, set()
        self.trace = self.levels = None
        self.last_submitted = None
        self.ev = trace_ref.evaluated(plan["n"], plan["dc_ignore_bins"], plan["use_bandwidth"])
        self.seen = set()  # the conditions met so far (coverage's labels)
        self.ever = set()  # the folds whose accumulator was set at some time

    # -- what a step must return ------------------------------------------------------------------------------------------------------
    def reason(self, st):
        """None where the step is accepted, else (status, why)"""
        op, slot = st["op"], st.get("slot")
        history = op in ("set_history", "update_history", "get_history", "confirmed")
        if not (self.has_hits if history else self.can_trace):
            return capi.E_INVALID, "a hits-only fixed plan" if self.has_hits else "a plan without SCN_OUT_HITS"
        if op in ("update_history", "update_trace", "update_levels", "confirmed"):
            if slot in self.pending:
                return capi.E_STATE, "a pending slot"
            if slot not in self.last:
                return capi.E_STATE, "a slot never collected"
            if slot not in self.listed:
                return capi.E_STATE, "after set_table"
            sub = self.last[slot]
            if op == "update_trace" and self.trace is None or op == "update_levels" and self.levels is None:
                return capi.E_STATE, "dropped" if op in self.ever else "none set"
            if op == "update_history":
                if not self.rows:
                    return capi.E_STATE, "dropped" if op in self.ever else "none set"
                if sub["units"] > self.rows:
                    return capi.E_INVALID, "more units than rows"
                if sub["indexed"] and sub["units"] and self.rows not in (1, self.table["count"]):
                    return capi.E_STATE, "indexed, rows neither 1 nor the table's count"
                if self.folded.get(slot):
                    return capi.E_STATE, "folded twice"
            if op == "confirmed":
                if not self.folded.get(slot):
                    return capi.E_STATE, "not folded"
                if self.folded[slot] != self.epoch or not self.rows:
                    return capi.E_STATE, "after set_history" if slot in self.set_history_since else "after another slot's fold"
        if op == "merge_trace":
            if self.trace is None:
                return capi.E_STATE, "none set"
            if st["nan"] is not None:
                return capi.E_INVALID, "a NaN in the window"
        if op == "emitters" and self.trace is None:
            return capi.E_STATE, "none set"
        return None

    def status(self, st):
        r = self.reason(st)
        return capi.OK if r is None else r[0]

    # -- what a step leaves --------------------------------------------------------------------------------------------------------------
    def _cells_of(self, geometry, centre):
        f = trace_ref.bin_freqs(self.plan["n"], FS, centre)[self.ev]
        below = f < np.uint64(geometry["f0"])
        c = (f[~below] - np.uint64(geometry["f0"])) // np.uint64(geometry["cell_hz"])
        inside = c < np.uint64(geometry["cells"])
        return bool(below.any()), bool((~inside).any()), np.unique(c[inside]).astype(np.int64)

    def _fold(self, st):
        op, slot, seen = st["op"], st["slot"], self.seen
        sub = self.last[slot]
        k, what = self.plan["average"], op.split("_")[1]
        seen.add(("fold", what, "overlap" if self.plan["overlap"] else "no overlap"))
        if not sub["units"]:
            seen.add(("fold", what, "zero units"))
        if sub["units"] and sub["units"] < self.before.get(slot, 0):
            seen.add(("fold", what, "smaller resubmit"))
        if self.pending:
            seen.add(("fold", what, "another slot pending"))
        if slot != self.last_submitted:
            seen.add(("fold", what, "not the last slot submitted"))
        if sub["indexed"] and k > 1 and any(g * (k - 1) % self.table["count"] for g in range(sub["units"])):
            seen.add(("fold", what, "averaged indexed"))
        if sub["indexed"] and sub["units"] and sub["first_index"] % max(1, self.rows) and op == "update_history":
            seen.add(("fold", what, "first_index"))
        if sub.get("out"):
            seen.add(("fold", what, "the caller's buffer"))
        for w, _ in sub["specials"].values():
            seen.add(("fold", what, "special", w))
        if op == "update_history":
            self.epoch += 1
            self.folded[slot] = self.epoch
            self.set_history_since.discard(slot)
            return
        if op == "update_levels":
            self.levels["fed"].add((slot, sub["seed"]))
        if op == "update_trace":
            t = self.trace
            t["fed"].add((slot, sub["seed"]))
            if t["was_reset_after_a_fold"]:
                seen.add(("trace", "a reset between folds"))
            t["folds"] += 1
            nan = {int(u) for u, (w, _) in sub["specials"].items() if w == "nan"}
            centres = unit_centres(self.plan, sub, self.table)
            for u in range(sub["units"]):
                if u in nan:
                    continue
                below, above, cells = self._cells_of(t, centres[u])
                if below:
                    seen.add(("trace", "bins below f0"))
                if above:
                    seen.add(("trace", "bins above the last cell"))
                if (t["unit"][cells] == t["folds"]).any():
                    seen.add(("trace", "a cell of two units of one submit"))
                t["unit"][cells] = t["folds"]
                if ((t["slots"][cells] != 0) & (t["slots"][cells] != 1 << slot)).any():
                    seen.add(("trace", "a cell of two slots"))
                t["slots"][cells] |= 1 << slot
                t["count"][cells] += 1
        if self.trace is not None and self.levels is not None and self.trace["fed"] & self.levels["fed"] and \
                any(self.trace[key] != self.levels[key] for key in ("f0", "cell_hz", "cells")):
            seen.add(("geometry", "levels and trace differ, fed by one submit"))

    def feed(self, st):
        op, slot, seen = st["op"], st.get("slot"), self.seen
        r = self.reason(st) if op in NEW_OPS else None
        if op in NEW_OPS:
            assert st["expect"] == (capi.OK if r is None else r[0]), (st, r)
        if st["expect"] != capi.OK:
            if r is not None:
                seen.add(("refusal", op, r[1]))
            return
        if op in ("set_history", "set_trace", "set_levels") and st.get("rows", st.get("cells")):
            self.ever.add("update_" + op[4:])
        if op == "submit":
            self.pending.append(slot)
            if slot in self.sub or slot in self.last:
                self.before[slot] = self.last.get(slot, {"units": 0})["units"]
            self.sub[slot] = st
            self.listed.discard(slot)
            self.last_submitted = slot
        elif op in ("collect", "counts"):
            self.pending.remove(slot)
            self.last[slot] = self.sub.pop(slot)
            self.folded[slot] = 0
            if self.has_hits:
                self.listed.add(slot)
        elif op == "set_table":
            self.table = st
            self.listed.clear()
        elif op == "set_history":
            self.epoch += 1
            self.rows = st["rows"]
            self.set_history_since |= {s for s, e in self.folded.items() if e}
            seen.add(("set_history", "slots pending" if self.pending else "no slot pending"))
            seen.add(("set_history", "rows", "table" if self.table and st["rows"] == self.table["count"] else "0" if not st["rows"] else "other"))
        elif op in ("update_history", "update_trace", "update_levels"):
            self._fold(st)
        elif op == "confirmed":
            if st["first"] > 1.0:
                seen.add(("confirmed", "past the end"))
            seen.add(("confirmed", st["m"], st["window"]))
        elif op == "set_trace":
            old = self.trace
            if st["cells"]:
                self.trace = dict(f0=st["f0"], cell_hz=st["cell_hz"], cells=st["cells"], count=np.zeros(st["cells"], np.int64), slots=np.zeros(st["cells"], np.int64),
                                  unit=np.zeros(st["cells"], np.int64), folds=0, fed=set(), merged=False, was_reset_after_a_fold=bool(old and old["folds"]))
                seen.add(("cells", "<64" if 1 < st["cells"] < 64 else st["cells"]))
                if old and all(old[key] == st[key] for key in ("f0", "cell_hz", "cells")) and (old["folds"] or old["merged"]):
                    seen.add(("set_trace", "the same geometry again"))
            else:
                self.trace = None
                seen.add(("set_trace", "dropped"))
        elif op == "set_levels":
            old = self.levels
            if st["cells"]:
                self.levels = dict(f0=st["f0"], cell_hz=st["cell_hz"], cells=st["cells"], edges=st["edges"], fed=set())
                seen.add(("edges", st["edges"]))
                if old and all(old[key] == st[key] for key in ("f0", "cell_hz", "cells", "edges")) and old["fed"]:
                    seen.add(("set_levels", "the same geometry again"))
            else:
                self.levels = None
                seen.add(("set_levels", "dropped"))
        elif op == "merge_trace":
            self.trace["count"][st["first"]:st["first"] + st["cells"]] += merge_window(st)[2].astype(np.int64)
            self.trace["merged"] = True
        elif op in ("get_trace", "emitters"):
            t = self.trace
            lo, hi = st["first_cell"], st["first_cell"] + st["cells"]
            occupied = np.flatnonzero(t["count"][lo:hi])
            if occupied.size and occupied.size < occupied[-1] - occupied[0] + 1:
                seen.add(("trace", "an empty cell inside, read"))
            if op == "emitters":
                seen.add(("line", st["line"]))
                seen.add(("max_gap", "cells" if st["max_gap"] == t["cells"] else st["max_gap"]))
                seen.add(("threshold", "tone" if st["level"] > 5.0 else "noise"))
                if st["first"] > 1.0:
                    seen.add(("emitters", "past the end"))
                if t["merged"]:
                    seen.add(("emitters", "after a merge"))
                if 0 < lo or hi < t["cells"]:
                    seen.add(("emitters", "a window of the trace"))
                # (a run across the seam of two 1024-cell tiles, as far as the script alone can tell: cells that units were folded into on
                # either side of it inside the window, the max line, a threshold below the noise's median, every gap bridged;
                # tests/sequence_run.py counts the records that do cross it)
                if lo <= 1023 and hi > 1024 and t["unit"][lo:1024].any() and t["unit"][1024:hi].any() and st["line"] == capi.TRACE_LINE_MAX and st["level"] < 0.0 \
                        and st["max_gap"] == t["cells"]:
                    seen.add(("emitters", "across the 1024-cell seam"))
        if op in NEW_OPS:
            seen.add(("op", op))


class _Extra:
    """the second pass over one script of the first"""

    def __init__(self, plan, steps, rng):
        self.plan, self.old, self.rng = plan, steps, rng
        self.t = Track(plan)
        self.out, self.n_new = [], 0
        self.top = plan["max_batch"] // plan["average"]
        self.want = dict(history=rng.random() < 0.75, trace=rng.random() < 0.85, levels=rng.random() < 0.7)
        self.same_grid = rng.random() < 0.3
        self.geometry = None

    def add(self, op, **kw):
        if self.n_new >= MAX_NEW_STEPS:
            return -1  # (the budget is spent: not added)
        st = dict(op=op, expect=capi.OK, **kw)
        st["expect"] = int(self.t.status(st))
        self.out.append(st)
        self.t.feed(st)
        self.n_new += 1
        return st["expect"]

    # -- what is drawn ------------------------------------------------------------------------------------------------------------------
    def _target(self, at):
        """the accepted submit whose centres a grid is laid over: the next one with units, else the last"""
        table, found = self.t.table, None
        for st in self.old[at:]:
            if st["op"] == "set_table" and st["expect"] == capi.OK:
                table = st
            if st["op"] == "submit" and st["expect"] == capi.OK and st["units"]:
                return unit_centres(self.plan, st, table)
        for st in self.old[:at]:
            if st["op"] == "set_table" and st["expect"] == capi.OK:
                table = st
            if st["op"] == "submit" and st["expect"] == capi.OK and st["units"]:
                found = unit_centres(self.plan, st, table)
        return np.array([100e6]) if found is None else found

    def grid(self, at, counts):
        """(f0, cell_hz, cells): the first unit's band starts below f0, and the last cell ends inside a unit's band"""
        rng = self.rng
        centres = np.sort(self._target(at))
        cells = int(rng.choice(counts))
        f0 = int(centres[0]) - int(rng.choice([1500000, 700000, 2100000]))
        last = centres[int(rng.integers(centres.size))] if rng.random() < 0.7 else centres[min(1, centres.size - 1)]
        end = int(last) + int(rng.choice([900000, -400000, 1700000]))
        return f0, max(1, (end - f0) // cells), cells

    def set_history(self):
        t, rng = self.t, self.rng
        rows = [0, 1, self.top, self.top + 2] + ([t.table["count"]] * 3 if t.table else [])
        self.add("set_history", rows=int(rng.choice(rows)))

    def set_trace(self, at, again=False):
        t = self.t
        if again and t.trace is not None and self.rng.random() < 0.5:
            return self.add("set_trace", f0=t.trace["f0"], cell_hz=t.trace["cell_hz"], cells=t.trace["cells"])
        f0, cell_hz, cells = self.grid(at, CELL_COUNTS)
        self.geometry = (f0, cell_hz, cells)
        return self.add("set_trace", f0=f0, cell_hz=cell_hz, cells=cells)

    def set_levels(self, at, again=False):
        t, rng = self.t, self.rng
        if again and t.levels is not None and rng.random() < 0.5:
            return self.add("set_levels", f0=t.levels["f0"], cell_hz=t.levels["cell_hz"], cells=t.levels["cells"], edges=t.levels["edges"])
        edges = str(rng.choice(EDGE_KINDS))
        if self.same_grid and t.trace is not None and t.trace["cells"] <= 200:
            f0, cell_hz, cells = t.trace["f0"], t.trace["cell_hz"], t.trace["cells"]
        else:
            f0, cell_hz, cells = self.grid(at, LEVEL_CELLS)
        return self.add("set_levels", f0=f0, cell_hz=cell_hz, cells=cells, edges=edges)

    def confirmed(self, slot):
        m, window = CONFIRMS[int(self.rng.integers(len(CONFIRMS)))]
        self.add("confirmed", slot=slot, m=m, window=window, first=float(self.rng.choice([0.0, 0.37, 0.61, 1.1])), cap=float(self.rng.choice([0.21, 0.5, 1.0])))

    def emitters(self):
        t, rng = self.t.trace, self.rng
        line = int(rng.choice(LINES))
        level = float(rng.choice([2.0, 6.0, 12.0])) if line == capi.TRACE_LINE_SPREAD else float(rng.choice([-3.0, -3.0, 1.0, 6.0, 10.0]))
        gap = rng.choice(len(GAPS))
        first_cell, cells = 0, t["cells"]
        if cells > 1025 and rng.random() < 0.4:  # across the seam of two tiles, every gap bridged
            first_cell, line, level, gap = int(rng.integers(0, 1024)), capi.TRACE_LINE_MAX, -3.0, GAPS.index("cells")
            cells -= first_cell
        elif cells > 2 and rng.random() < 0.5:  # a window that may start or end inside a run
            first_cell = int(rng.integers(0, cells // 2))
            cells = int(rng.integers(1, cells - first_cell + 1))
        self.add("emitters", line=line, level=level, max_gap=t["cells"] if GAPS[gap] == "cells" else int(GAPS[gap]), first_cell=first_cell, cells=cells,
                 first=float(rng.choice([0.0, 0.37, 0.61, 1.1])), cap=float(rng.choice([0.21, 0.5, 1.0])))

    def merge(self, nan=False):
        t, rng = self.t.trace, self.rng
        first = int(rng.integers(0, t["cells"]))
        cells = int(rng.integers(1, t["cells"] - first + 1))
        if t["cells"] >= 1025 and rng.random() < 0.6:  # over the seam of two tiles
            first = int(rng.integers(900, 1020))
            cells = t["cells"] - first
        self.add("merge_trace", first=first, cells=cells, seed=int(rng.integers(1 << 30)), nan=int(rng.integers(0, 2 * cells)) if nan else None)

    def reads(self, share=0.5):
        t, rng = self.t, self.rng
        if t.trace is not None and rng.random() < share:
            if rng.random() < 0.5:
                self.add("get_trace", first_cell=0, cells=t.trace["cells"])
            else:
                first = int(rng.integers(0, t.trace["cells"]))
                self.add("get_trace", first_cell=first, cells=int(rng.integers(0, t.trace["cells"] - first + 1)))
        for _ in range(int(rng.integers(0, 3)) if t.trace is not None else 0):
            self.emitters()
        if t.levels is not None and rng.random() < share:
            self.add("get_levels")
        if t.levels is not None and rng.random() < share:
            n_edges = edges_of(self.plan, t.levels["edges"]).size
            self.add("levels_summary", permille=int(rng.choice([0, 250, 500, 999, 1000])), level=int(rng.choice([0, n_edges // 2, n_edges])))
        if t.has_hits and t.rows and rng.random() < share:
            self.add("get_history")

    def folds(self, slot, share=0.85):
        """the folds of one slot, in a drawn order; a confirmation behind an accepted fold into the history"""
        t, rng = self.t, self.rng
        for what in rng.permutation(["history", "trace", "levels"]):
            if not self.want[str(what)] and rng.random() < 0.9 or rng.random() > share:
                continue
            st = self.add("update_" + str(what), slot=slot)
            if what == "history" and st == capi.OK:
                for _ in range(int(rng.integers(1, 3))):
                    self.confirmed(slot)
                if rng.random() < 0.25:
                    self.add("update_history", slot=slot)  # (once per submit)
            elif what != "history" and st == capi.OK and rng.random() < 0.15:
                self.add("update_" + str(what), slot=slot)  # (twice is allowed: it counts twice)

    # -- the pass ---------------------------------------------------------------------------------------------------------------------
    def setup(self, at):
        t = self.t
        if self.want["history"] and t.has_hits:
            self.set_history()
        if self.want["trace"] and t.can_trace:
            self.set_trace(at)
        if self.want["levels"] and t.can_trace:
            self.set_levels(at)

    def run(self):
        t, rng, old = self.t, self.rng, self.old
        late = rng.random() < 0.25  # nothing is set until the first collect: a fold before that finds none
        if not t.has_hits:
            self.add("set_history", rows=2)
        if not t.can_trace:
            self.add("set_trace", f0=99000000, cell_hz=100000, cells=64)
            if rng.random() < 0.5:
                self.add("set_levels", f0=99000000, cell_hz=100000, cells=8, edges="few")
        if not late:
            self.setup(0)
        if t.has_hits and rng.random() < 0.3:
            self.add(str(rng.choice(["update_history", "update_trace", "update_levels"])), slot=int(rng.integers(capi.NUM_SLOTS)))  # never collected
        done_setup = not late
        for at, st in enumerate(old):
            ok = st["expect"] == capi.OK
            if ok and st["op"] == "submit" and not st["pinned"] and st["units"] and self.plan["flags"] & capi.OUT_SPECTRUM and rng.random() < 0.4:
                st = dict(st, out=True)  # the spectrum goes into the caller's device buffer
            self.out.append(st)
            t.feed(st)
            if not ok or not t.has_hits:
                continue
            op, slot = st["op"], st.get("slot")
            if op == "submit":
                if rng.random() < 0.15:
                    self.add(str(rng.choice(["update_history", "update_trace", "update_levels"])), slot=slot)  # a pending slot
                if self.want["history"] and rng.random() < 0.12:
                    self.set_history()
                if t.can_trace and rng.random() < 0.08:
                    self.set_trace(at, again=True)
                if t.can_trace and rng.random() < 0.06:
                    self.set_levels(at, again=True)
                if t.trace is not None and rng.random() < 0.12:
                    self.merge(nan=rng.random() < 0.3)
                if t.listed and rng.random() < 0.2:
                    self.folds(int(rng.choice(sorted(t.listed))), 0.6)  # with this slot pending, and not the last one submitted
                if rng.random() < 0.15:
                    self.reads(0.4)
            elif op in ("collect", "counts"):
                if not done_setup:
                    if rng.random() < 0.7:
                        self.add(str(rng.choice(["update_history", "update_trace", "update_levels"])), slot=slot)  # none set
                    self.setup(at + 1)
                    done_setup = True
                if rng.random() < 0.8:
                    self.folds(slot)
                others = sorted(t.listed - {slot})
                if others and rng.random() < 0.35:
                    other = int(rng.choice(others))
                    self.folds(other, 0.7)
                    if t.folded.get(slot) and t.folded.get(other, 0) > t.folded[slot]:
                        self.confirmed(slot)  # another slot was folded since
                if t.folded.get(slot) == t.epoch and t.rows and rng.random() < 0.2:
                    self.set_history()
                    self.confirmed(slot)  # after set_history
                if t.trace is not None and rng.random() < 0.2:
                    self.merge(nan=rng.random() < 0.25)
                self.reads()
                if t.can_trace and rng.random() < 0.1:
                    (self.set_trace if rng.random() < 0.6 else self.set_levels)(at + 1, again=True)
                if t.can_trace and rng.random() < 0.04:
                    self.add("set_trace", f0=0, cell_hz=0, cells=0) if rng.random() < 0.5 else self.add("set_levels", f0=0, cell_hz=0, cells=0, edges="one")
            elif op == "set_table":
                gone = sorted(t.last)
                if gone and rng.random() < 0.6:
                    self.add(str(rng.choice(["update_history", "update_trace", "update_levels"])), slot=int(rng.choice(gone)))  # the list is gone
                if self.want["history"] and rng.random() < 0.6:
                    self.add("set_history", rows=st["count"])
        self.reads(0.8)
        return dict(plan=self.plan, steps=self.out)


def draw(seed):
    """the plan scripts of one seed"""
    first = [_Gen(np.random.default_rng([int(seed), index])).run() for index in range(SCRIPTS_PER_SEED)]
    return [_Extra(sc["plan"], sc["steps"], np.random.default_rng([int(seed), index, 1])).run() for index, sc in enumerate(first)]


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
        track = Track(plan)  # (the second pass's conditions)
        learnt, submitted, nan_units = False, set(), set()  # the baseline holds finite rows; slots with something to fold; slots whose last submit has a NaN unit
        for st in steps:
            op, ok = st["op"], st["expect"] == capi.OK
            track.feed(st)
            if op in NEW_OPS:
                continue
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
        got |= track.seen
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
    # the second pass: the hit history, the sweep trace, the level histogram, the trace emitters
    folds = ("update_history", "update_trace", "update_levels")
    need |= {("op", o) for o in NEW_OPS}
    need |= {("refusal", o, why) for o in folds for why in ("a pending slot", "a slot never collected", "after set_table", "none set")}
    need |= {("refusal", "update_history", why) for why in ("folded twice", "more units than rows", "indexed, rows neither 1 nor the table's count")}
    need |= {("refusal", "confirmed", why) for why in ("after another slot's fold", "after set_history")}
    need |= {("refusal", o, "dropped") for o in folds}
    need |= {("refusal", "set_history", "a plan without SCN_OUT_HITS"), ("refusal", "set_trace", "a plan without SCN_OUT_HITS"),
             ("refusal", "set_trace", "a hits-only fixed plan"), ("refusal", "merge_trace", "a NaN in the window")}
    need |= {("fold", w, c) for w in ("history", "trace", "levels")
             for c in ("smaller resubmit", "zero units", "another slot pending", "not the last slot submitted", "averaged indexed", "overlap", "no overlap")}
    need |= {("fold", w, "special", sp) for w in ("trace", "levels") for sp in ("nan", "overflow", "zero")}
    need |= {("fold", "trace", "the caller's buffer"), ("fold", "levels", "the caller's buffer"), ("fold", "history", "first_index")}
    need |= {("trace", c) for c in ("bins below f0", "bins above the last cell", "a cell of two units of one submit", "a cell of two slots", "an empty cell inside, read",
                                    "a reset between folds")}
    need |= {("geometry", "levels and trace differ, fed by one submit"), ("set_trace", "the same geometry again"), ("set_levels", "the same geometry again"),
             ("set_trace", "dropped"), ("set_levels", "dropped")}
    need |= {("set_history", c) for c in ("slots pending", "no slot pending")} | {("set_history", "rows", r) for r in ("table", "0", "other")}
    need |= {("cells", c) for c in (1, "<64", 1023, 1024, 1025)} | {("edges", e) for e in EDGE_KINDS} | {("line", l) for l in LINES} | {("max_gap", g) for g in GAPS}
    need |= {("threshold", "noise"), ("threshold", "tone"), ("emitters", "past the end"), ("emitters", "after a merge"), ("emitters", "a window of the trace"),
             ("emitters", "across the 1024-cell seam"), ("confirmed", "past the end")} | {("confirmed", m, w) for m, w in CONFIRMS}
    return need


def search_seeds(candidates=range(4000), cost=None, start=()):
    """a greedy cover of required() by seeds (how SEEDS was chosen): repeatedly the seed that covers most of what is still missing;
    start: the seeds that stay, in front"""
    need, chosen = required(), list(start)
    for s in start:
        need -= coverage(draw(s))
    covers = {s: coverage(draw(s)) & need for s in candidates}
    while need:
        best = max(covers, key=lambda s: (len(covers[s] & need), -s))
        if not covers[best] & need:
            raise AssertionError(f"no candidate covers {sorted(need, key=str)}")
        chosen.append(best)
        need -= covers[best]
    return chosen
