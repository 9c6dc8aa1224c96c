"""The two readings of a post's headers, held to each other on the CPU: scn_stream_outcome (scn_gather_protocol.h, what
scn_gather_wait reports and what the compaction kernel is held to by tests/test_gather_kernels_gpu.py) and sweep.stream_outcome
(the restatement the world-2 / 3 / 8 gloo tests pass or fail by).  tests/cpp/test_gather_protocol.cpp --outcomes prints the C
reading of seeded header sets; the Python twin must agree on everything they both report: status, the first bad rank, what it
announced, the step, the ranks' counts, the offsets and the total."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from scanner_amd import capi, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICKETS = capi.GATHER_TICKETS


def _good(rng, cap, seq):
    count = int(rng.choice([0, 1, cap - 1, cap, int(rng.integers(0, cap + 1))]))
    return [count, capi.OK, count, sweep.STREAM_MAGIC, seq]


def _defects(cap, seq):
    """Every way a header can differ from a good one: name -> edit of [count, status, sent, magic, seq]."""
    def edit(**kw):
        def f(h):
            for k, v in kw.items():
                h[{"count": 0, "status": 1, "sent": 2, "magic": 3, "seq": 4}[k]] = (v(h) if callable(v) else v) % (1 << (64 if k == "seq" else 32))
        return f
    return {
        "magic": edit(magic=sweep.STREAM_MAGIC ^ 0x10000),
        "magic_zero": edit(magic=0),
        "seq_minus_1": edit(seq=(seq - 1) % (1 << 64)),
        "seq_plus_1": edit(seq=(seq + 1) % (1 << 64)),
        "seq_minus_tickets": edit(seq=(seq - TICKETS) % (1 << 64)),
        "seq_high_word": edit(seq=seq ^ (1 << 32)),
        "sent_cap_plus_1": edit(sent=cap + 1, count=cap + 1),
        "sent_above_count": edit(count=lambda h: min(h[0], cap - 1), sent=lambda h: h[0] + 1),   # (in this order: sent = the new count + 1 <= cap)
        "sent_max": edit(sent=0xFFFFFFFF),
        "sent_and_count_max": edit(sent=0xFFFFFFFF, count=0xFFFFFFFF),
        "failed_empty": edit(status=capi.E_NOMEM, count=0, sent=0),
        "failed_with_records": edit(status=capi.E_STATE),
        "truncated_nothing_cut": edit(status=capi.E_TRUNCATED),
        "truncated": edit(status=capi.E_TRUNCATED, count=cap + 7, sent=cap),
        "truncated_count_max": edit(status=capi.E_TRUNCATED, count=0xFFFFFFFF, sent=cap),
        "cut_but_status_ok": edit(count=lambda h: h[2] + 3),
        "status_unknown": edit(status=0xFFFFFFFF),
    }


def _header_sets():
    rng = np.random.default_rng(20240607)
    sets = []
    # every defect at every position of every world, beside good neighbours
    for world in range(1, 9):
        cap, seq = 10, (1 << 32) + 41 + world
        for name in _defects(cap, seq):
            for pos in range(world):
                heads = [_good(rng, cap, seq) for _ in range(world)]
                _defects(cap, seq)[name](heads[pos])
                sets.append((cap, seq, heads))
    # combinations: several defects in one header, several spoiled ranks in one set
    while len(sets) < 4000:
        world = int(rng.integers(1, 9))
        cap = int(rng.choice([1, 2, 10, 300, 11000]))
        seq = [0, 1, 3, 4, 5, (1 << 32) - 1, 1 << 32, (1 << 32) + 6, (1 << 64) - 1][int(rng.integers(0, 9))]
        d = _defects(cap, seq)
        names = list(d)
        heads = [_good(rng, cap, seq) for _ in range(world)]
        for h in heads:
            if rng.random() < 0.4:
                for name in rng.choice(names, size=int(rng.integers(1, 4)), replace=False):
                    d[name](h)
        sets.append((cap, seq, heads))
    return sets


@pytest.fixture(scope="module")
def c_reading(tmp_path_factory):
    """(the header sets, scn_stream_outcome's reading of each as a list of ints)."""
    d = tmp_path_factory.mktemp("gather_twin")
    exe = d / "test_gather_protocol"
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-g", "-pthread", "-I", os.path.join(ROOT, "scanner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_gather_protocol.cpp"), "-o", str(exe)])
    sets = _header_sets()
    with open(d / "sets.txt", "w") as fh:
        for cap, seq, heads in sets:
            fh.write(f"{cap} {seq} {len(heads)} " + " ".join(" ".join(str(v) for v in h) for h in heads) + "\n")
    out = subprocess.run([str(exe), "--outcomes", str(d / "sets.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [[int(v) for v in ln.split()] for ln in out.stdout.splitlines()]
    assert len(lines) == len(sets)
    return sets, lines


def _heads_array(heads):
    a = np.zeros(len(heads), sweep.STREAM_HEAD)
    for k, f in enumerate(("count", "status", "sent", "magic", "seq")):
        a[f] = np.array([h[k] for h in heads], dtype=sweep.STREAM_HEAD[f])
    return a


def _disagreements(twin, sets, lines):
    bad = []
    for k, ((cap, seq, heads), c) in enumerate(zip(sets, lines)):
        world = len(heads)
        o = twin(_heads_array(heads), cap, seq)
        got = [int(o.status), int(o.bad_rank), int(o.bad_status), int(o.step), int(o.offsets[world])] + [int(v) for v in o.per_rank] + [int(v) for v in o.offsets]
        if got != c:
            bad.append((k, cap, seq, heads, got, c))
    return bad


def test_the_sets_cover_what_they_claim(c_reading):
    sets, lines = c_reading
    assert len(sets) >= 4000 and {len(h) for _, _, h in sets} == set(range(1, 9))
    statuses = {ln[0] for ln in lines}
    assert statuses == {capi.OK, capi.E_TRUNCATED, capi.E_COMM}              # every class of outcome occurs ...
    assert {ln[3] for ln in lines if ln[0] == capi.E_COMM} == {1, 3}         # ... both kinds of E_COMM ...
    for world in range(1, 9):                                                 # ... and every rank of every world is the bad one somewhere
        assert {ln[1] for (_, _, h), ln in zip(sets, lines) if len(h) == world} >= set(range(-1, world))
    assert sum(ln[0] == capi.OK for ln in lines) > 100


def test_python_twin_reads_headers_as_scn_stream_outcome_does(c_reading):
    sets, lines = c_reading
    bad = _disagreements(sweep.stream_outcome, sets, lines)
    assert not bad, f"{len(bad)} of {len(sets)} sets; the first: set {bad[0][0]} cap {bad[0][1]} seq {bad[0][2]} heads {bad[0][3]}: twin {bad[0][4]}, C {bad[0][5]}"


def _broken_twin(old, new):
    src = inspect.getsource(sweep.stream_outcome)
    assert src.count(old) == 1, old
    scope = dict(vars(sweep))
    exec(src.replace(old, new), scope)
    return scope["stream_outcome"]


@pytest.mark.parametrize("old,new", [
    (" and sent <= count", ""),                                    # the `sent <= count` clause skipped
    ("per_rank[r] = count if intact else 0", "per_rank[r] = count"),  # a non-intact rank's count counted
    (" and sent <= cap", ""),
    ("hseq == seq % (1 << 64)", "hseq % (1 << 32) == seq % (1 << 32)"),
    ("status, bad_rank, bad_status, step = capi.E_COMM, r, st, 1", "status, bad_rank, bad_status, step = capi.E_COMM, r, st, 3"),
], ids=["no_sent_le_count", "counts_a_bad_rank", "no_sent_le_cap", "seq_low_word_only", "step_of_a_marked_rank"])
def test_a_broken_twin_is_caught(c_reading, old, new):
    """The differential test can fail: each of these one-line edits of the twin disagrees with the C reading on some set."""
    sets, lines = c_reading
    assert _disagreements(_broken_twin(old, new), sets, lines)
