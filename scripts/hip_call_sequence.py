"""Which HIP runtime calls one step of a submit / collect loop makes, shape by shape -- the evidence that a change to the C-ABI
layer's host code left its calls as they were (steps of 16 ... 128 points are bound by them, 4 - 5 us each).

  rocprofv3 --hip-trace --output-format csv -d OUT -- python scripts/hip_call_sequence.py run     # (SCN_LIB selects the library)
  python scripts/hip_call_sequence.py extract OUT > calls.txt                                     # one line per shape

`run` drives, per shape, a two-slot loop of 20 steps through scanner_amd.capi (collect the slot's previous submit, submit) and
brackets the 10th step with two calls of hipRuntimeGetVersion, which the library never makes.  `extract` reads the trace's
*hip_api_trace.csv and prints the API names between the two marks of every shape.  Tracing slows every call: no timing."""
import csv
import ctypes as C
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MARK = "hipRuntimeGetVersion"
# name, n, kind, buffers per submit, plan fields, collect records?
SHAPES = [("direct counts 4096 cfloat x 2048", 4096, 4, 2048, {}, False),
          ("eager list 4096 cfloat x 8192", 4096, 4, 8192, {}, True),
          ("total_path 16 cfloat x 262144", 16, 4, 262144, {}, False),
          ("average 2, 1024 x 8", 1024, 4, 8, {"average": 2}, False),
          ("floor 64 x 8", 64, 4, 8, {"detect": 1, "threshold": 6.0}, False),
          ("overlapped slots 4096 int16 x 64", 4096, 3, 64, {"flags": 1 | 2 | 4}, False),
          ("floor 64 x 3000, records", 64, 4, 3000, {"detect": 1, "threshold": 6.0}, True),  # not fused, eager, counts by DMA
          ("spectrum only 4096 cfloat x 8192", 4096, 4, 8192, {"flags": 1}, False)]  # `done` completed by the dispatch packet


def run():
    import numpy as np
    import torch

    from scanner_amd import capi

    L, VP = capi.lib(), C.c_void_p
    with open("/proc/self/maps") as fh:  # the HIP runtime this process already uses (torch's), for the marks
        hip = C.CDLL(next(line.split()[-1] for line in fh if "libamdhip64" in line))
    version = C.c_int()
    rng = np.random.default_rng(3)
    for name, n, kind, nb, fields, records in SHAPES:
        fields = dict(fields)
        d = capi.PlanDesc(struct_size=C.sizeof(capi.PlanDesc), n=n, sample_rate=8000000, sample_kind=kind, enob=12,
                          threshold=fields.pop("threshold", 14.0), max_batch=nb, max_hits=1 << 16, **fields)
        plan = VP()
        capi.check(L.scn_plan_create(C.byref(d), C.byref(plan)), "scn_plan_create")
        x = rng.standard_normal(2 * n * nb).astype(np.float32)
        raw = torch.from_numpy(x if kind == 4 else (x * 300).astype(np.int16)).cuda()
        units = nb // max(d.average, 1)
        fc = np.repeat(1e8 + 6e6 * np.arange(units), nb // units)
        hits, total = np.empty(1 << 16, capi.HIT_DTYPE), C.c_uint32()
        torch.cuda.synchronize()
        for step in range(20 + 2):
            slot = step % 2
            if step == 10 or step == 11:
                hip.hipRuntimeGetVersion(C.byref(version))
            if step >= 2:
                st = L.scn_collect(plan, slot, None, hits.ctypes.data_as(VP) if records else None, hits.size, C.byref(total), None)
                if st != capi.E_TRUNCATED:
                    capi.check(st, "scn_collect")
            if step < 20:
                capi.check(L.scn_submit_device(plan, slot, raw.data_ptr(), nb, fc.ctypes.data_as(VP), None, None), "scn_submit_device")
        print(f"{name}: {total.value} hits in the last step", flush=True)
        capi.check(L.scn_plan_destroy(plan), "scn_plan_destroy")


def extract(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*hip_api_trace.csv"), recursive=True):
        with open(path) as fh:
            rows += [(int(r["Start_Timestamp"]), r["Function"]) for r in csv.DictReader(fh)]
    names = [f for _, f in sorted(rows)]
    marks = [k for k, f in enumerate(names) if f == MARK]
    assert len(marks) >= 2 * len(SHAPES), f"{len(marks)} marks in the trace, {2 * len(SHAPES)} expected"
    marks = marks[-2 * len(SHAPES):]  # (whatever the process called while it started up comes before)
    for s, shape in enumerate(SHAPES):
        print(f"{shape[0]}: " + " ".join(names[marks[2 * s] + 1:marks[2 * s + 1]]))


if __name__ == "__main__":
    run() if sys.argv[1:2] == ["run"] else extract(sys.argv[2])
