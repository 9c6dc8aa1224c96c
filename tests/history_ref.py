"""A numpy model of the hit history (include/scanner_hip.h, "Hit history"), written from the definition and not from the C code.

history[rows, n] uint32 by fftshift index i, visits[rows] uint32.  Bit 0 of a word is the row's most recent visit.  A submit's
ordered hit list (capi.HIT_DTYPE) is split among its units by seq_id: unit u owns the records whose seq_id is unit_ids[u] -- the
ids of a submit's units are distinct in every scene the tests make, so a mask does what the C forms' cursor does."""
import numpy as np


def new(rows, n):
    return np.zeros((rows, n), np.uint32), np.zeros(rows, np.uint32)


def unit_ids(n_units, seq_ids=None):
    return np.arange(n_units, dtype=np.uint64) if seq_ids is None else np.asarray(seq_ids, np.uint64)


def _unit_of(ids, seq):
    """the unit whose id each record carries (the ids are distinct)"""
    order = np.argsort(ids)
    return order[np.searchsorted(ids[order], seq)] if len(seq) else np.zeros(0, np.int64)


def fold(history, visits, hits, n_units, first=0, seq_ids=None):
    """(history, visits) after the submit: every word of every unit's row shifts left by one and takes hit(u, i); the row's visits
    grow by one and stop at 0xffffffff.  Rows no unit maps to come back as they were.  The inputs are not written."""
    rows, n = history.shape
    assert n_units <= rows
    history, visits = history.copy(), visits.copy()
    ids = unit_ids(n_units, seq_ids)
    assert len(set(ids.tolist())) == n_units and np.isin(hits["seq_id"], ids).all()
    hit = np.zeros((n_units, n), np.uint64)  # hit(u, i)
    hit[_unit_of(ids, hits["seq_id"]), hits["i"]] = 1
    r = (int(first) + np.arange(n_units)) % rows  # (n_units <= rows: no row twice)
    history[r] = (((history[r].astype(np.uint64) << np.uint64(1)) | hit) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    visits[r] = np.minimum(visits[r].astype(np.uint64) + 1, 0xFFFFFFFF).astype(np.uint32)
    return history, visits


def popcount(words):
    return np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)


def confirm(history, hits, n_units, m, window, first=0, seq_ids=None):
    """the subsequence of `hits` whose history word has at least m of its `window` lowest bits set"""
    rows, n = history.shape
    assert 1 <= m <= window <= 32
    ids = unit_ids(n_units, seq_ids)
    r = (int(first) + _unit_of(ids, hits["seq_id"])) % rows
    mask = 0xFFFFFFFF if window == 32 else (1 << window) - 1
    words = history[r, hits["i"]] & np.uint32(mask)
    return hits[popcount(words) >= m]
