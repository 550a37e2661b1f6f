"""k_fused's pop over several stack entries per pass (csrc/pop_batch.h: ptpb::pop_first_within<N>) against the loop it replaced, without a GPU.

The rule: a pop takes the first entry from the top that is within the cut key (raw entry <= cut) and does not carry the lane's own leaf code;
the entries above it are gone with it; the BOTTOM entry (key +0 | DONE) is within every cut and ends the search.  tests/pop_batch_host.cpp
compiles the header for the host and pops every case in passes of N = 1, 2, 3 and 4 entries; the reference is the one-entry-at-a-time loop,
written here.  Code, entries gone and passes must agree for every case: every pattern of {behind the cut, within, within and the lane's own
leaf, equal to the cut's key} over stacks of up to five entries above BOTTOM -- so the first qualifying entry, BOTTOM and the own leaf stand at
every position of a pass -- with the distances and child words of tests/test_cut_key_cpu.py, cuts of +inf and FLT_MAX | 0x3FFF among them, and
words below BOTTOM that would qualify if anybody looked.  The second build runs the same cases under AddressSanitizer and UBSan.
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_cut_key_cpu as ck

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc")
U32 = np.uint32
PENDING, NO_SELF = U32(0xFFFFFFFF), U32(0xFFFFFFFF)
BEHIND, WITHIN, SELF, EQUAL = range(4)
MAX_LIVE, BELOW = 5, 3            # entries above BOTTOM; words below it (a pass of four that starts on BOTTOM reads three)
DEPTH = MAX_LIVE + 1 + BELOW
NS = (1, 2, 3, 4)


def _cuts():
    """cut keys as the kernel forms them: pop_cut and push_cut of the special distances and of a sample of the others"""
    v = ck.distances()
    rng = np.random.default_rng(11)
    b = np.concatenate([U32([0, 1, 0x3FFF, 0x4000, 0x00800000, 0x3F800000, ck.FLT_MAX_BITS - 1, ck.FLT_MAX_BITS, ck.INF_BITS]), rng.choice(v, 27)]).astype(U32)
    cuts = np.unique(np.concatenate([ck.pop_cut(b), ck.push_cut(b)]))
    assert U32(ck.INF_BITS | 0x3FFF) in cuts and U32(ck.FLT_MAX_BITS) in cuts     # +inf, and FLT_MAX | 0x3FFF (the cap)
    return cuts


def cases():
    """-> stack [n, DEPTH] (top entry first), cut [n], self [n], index of BOTTOM [n]"""
    keys = np.unique(ck.distances() & ck.KEY_MASK)            # sorted truncated distances, +0 first, +inf last
    cuts = _cuts()
    rng = np.random.default_rng(5)
    patterns = [p for live in range(MAX_LIVE + 1) for p in itertools.product(range(4), repeat=live)]
    n_p, n_c = len(patterns), len(cuts)
    cls = np.full((n_p, MAX_LIVE), -1, np.int64)
    live = np.zeros(n_p, np.int64)
    for k, p in enumerate(patterns):
        cls[k, :len(p)] = p
        live[k] = len(p)
    out = []
    for wmode in range(3):                                    # child words: all zero, all ones, random (test_cut_key_cpu.words)
        cl = np.repeat(cls, n_c, axis=0)
        lv = np.repeat(live, n_c)
        cut = np.tile(cuts, n_p).astype(U32)
        n = len(cut)
        self_code = (U32(0x2000) | (rng.integers(0, 2, n).astype(U32) << U32(11)) | rng.integers(0, 0x800, n).astype(U32)).astype(U32)
        self_code[rng.random(n) < 0.15] = NO_SELF             # (a kernel without the rule)
        n_within = np.searchsorted(keys, cut & ck.KEY_MASK, side="right")    # keys[:n_within] are within the cut (never empty: +0)
        stack = np.zeros((n, DEPTH), U32)
        for j in range(MAX_LIVE):
            c = cl[:, j]
            some_behind = n_within < len(keys)
            behind = (c == BEHIND) & some_behind              # (a cut of +inf has nothing behind it: such an entry is within)
            idx = np.where(behind, n_within + (rng.random(n) * (len(keys) - n_within)).astype(np.int64), (rng.random(n) * n_within).astype(np.int64))
            key = keys[np.minimum(idx, len(keys) - 1)]
            key = np.where(c == EQUAL, np.minimum(cut & ck.KEY_MASK, U32(ck.INF_BITS)), key).astype(U32)
            word = [np.zeros(n, U32), np.full(n, 0x3FFF, U32), rng.integers(0, 0x4000, n).astype(U32)][wmode]
            word = np.where((c == SELF) & (self_code != NO_SELF), self_code, word).astype(U32)
            stack[:, j] = np.where(c >= 0, key | word, 0)
        # BOTTOM under the live entries, then words that would qualify: +0 keys over small words, leaf codes, DONE; and any words at all
        rows = np.arange(n)
        below = np.stack([rng.choice(U32([0, 1, 2, 0x2000, 0x2001, 0x3FFF, 0x4000]), n), rng.integers(0, 0x4000, n).astype(U32),
                          rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U32)], axis=1)
        for k in range(BELOW):
            stack[rows, lv + 1 + k] = below[:, k]
        stack[rows, lv] = U32(ck.BOTTOM)
        out.append((stack, cut, self_code, lv))
    return [np.concatenate([o[k] for o in out]) for k in range(4)]


def one_at_a_time(stack, cut, self_code):
    """the loop the batched pop replaced: pop one entry, test it, again -> code, entries gone"""
    n = len(cut)
    r = np.full(n, PENDING, U32)
    gone = np.zeros(n, np.int64)
    for j in range(stack.shape[1]):
        pend = r == PENDING
        if not pend.any():
            break
        e = stack[:, j]
        gone[pend] += 1
        take = pend & (e <= cut) & ((e & ck.WORD_MASK) != self_code)
        r[take] = e[take] & ck.WORD_MASK
    assert (r != PENDING).all()
    return r, gone


@pytest.fixture(scope="module")
def want():
    stack, cut, self_code, bottom = cases()
    code, gone = one_at_a_time(stack, cut, self_code)
    for a in (stack, cut, self_code, bottom, code, gone):
        a.setflags(write=False)
    return stack, cut, self_code, bottom, code, gone


def test_the_cases_cover_the_places_where_the_forms_could_part(want):
    stack, cut, self_code, bottom, code, gone = want
    assert len(cut) > 100000
    assert (gone <= bottom + 1).all()                                     # nothing below BOTTOM is ever taken ...
    below = stack[np.arange(len(cut)), bottom + 1]
    assert ((below <= cut) & ((below & ck.WORD_MASK) != self_code)).mean() > 0.5   # ... though most of those words would qualify
    for pos in range(MAX_LIVE + 1):
        at = gone == pos + 1
        assert (at & (bottom == pos)).any() and (code[at & (bottom == pos)] == ck.DONE).all()     # BOTTOM taken at every position
        if pos < MAX_LIVE:
            assert (at & (bottom > pos)).any()                                                    # ... and a live entry
    live = np.arange(DEPTH)[None, :] < bottom[:, None]
    is_self = live & ((stack & ck.WORD_MASK) == self_code[:, None]) & (stack <= cut[:, None])
    above_taken = np.arange(DEPTH)[None, :] < (gone - 1)[:, None]
    for pos in range(MAX_LIVE):
        assert (is_self & above_taken)[:, pos].any()                      # the own leaf, within the cut, passed over at every position
    same = live[:, 1:] & (stack[:, 1:] == stack[:, :-1])
    assert same.any()                                                     # equal keys (and words) next to each other
    for c in (ck.INF_BITS | 0x3FFF, ck.FLT_MAX_BITS):
        assert (cut == U32(c)).sum() > 1000
    assert (gone > 4).any()                                               # more than one pass even of four entries


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_batched_pop_equals_the_one_entry_loop(tmp_path, want, sanitize):
    stack, cut, self_code, bottom, code, gone = want
    exe = str(tmp_path / "pop_batch_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", CSRC, "-I", os.path.join(REPO, "tests"), "-o", exe, os.path.join(REPO, "tests", "pop_batch_host.cpp")])
    d = str(tmp_path)
    U32([len(cut), DEPTH]).tofile(os.path.join(d, "par"))
    np.ascontiguousarray(stack).tofile(os.path.join(d, "stack"))
    cut.tofile(os.path.join(d, "cut"))
    self_code.tofile(os.path.join(d, "self"))
    subprocess.check_call([exe, d])
    pos = np.arange(DEPTH)[None, :]
    own_above = ((pos < (gone - 1)[:, None]) & (stack <= cut[:, None]) & ((stack & ck.WORD_MASK) == self_code[:, None])).sum(axis=1)
    for n in NS:
        got_code, got_gone, got_passes = (np.fromfile(os.path.join(d, f"o_{what}_{n}"), U32) for what in ("code", "pops", "passes"))
        bad = np.flatnonzero((got_code != code) | (got_gone != gone))
        assert len(bad) == 0, (n, len(bad), [hex(x) for x in stack[bad[0]]], hex(cut[bad[0]]), hex(self_code[bad[0]]), hex(got_code[bad[0]]), hex(code[bad[0]]))
        # passes: the taken entry's own, counted in full batches from the top -- except that a pass ends early at an entry within the cut that
        # is the lane's own leaf (the next pass starts below it): at most one pass more per such entry above the taken one
        full = (gone - 1) // n + 1
        assert (got_passes >= full).all() and (got_passes <= full + own_above).all() and (got_passes <= gone).all(), n
        assert (got_passes[own_above == 0] == full[own_above == 0]).all(), n
        if n > 1:
            assert (got_passes < gone).any()
    assert (code != PENDING).all()


def test_the_header_is_what_the_kernel_uses():
    """pop_pending goes through pop_first_within for every instantiation, and the LDS plan leaves room for the reads under BOTTOM"""
    fk = open(os.path.join(CSRC, "fused_kernel.h")).read()
    assert "ptpb::pop_first_within<POP_N>(e, kcut, SKIP ? self_leaf : ptpb::NO_SELF)" in fk
    assert "l.stack >= l.state + sizeof(uint32_t) * FTB * PT_FUSED_POP_N_MAX + 4u" in fk
    assert "static_assert(PT_FUSED_POP_N >= 1 && PT_FUSED_POP_N <= PT_FUSED_POP_N_MAX" in fk
    assert '#include "pop_batch.h"' in open(os.path.join(CSRC, "extend_kernel.h")).read()
