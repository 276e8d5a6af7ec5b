"""GPU: every kernel family behind every other one in the scratch arena they share, and on poisoned memory.

The arenas of a context (csrc/pvf_internal.h: `DevBuf s_*`) are grow-only and shared: nine families carve s_act0, seven s_trk0, six
s_clu0 / s_clu1, five s_misc, three s_chip, two s_chip_pyr (tests/scratch_cases.py: SHARERS).  A fresh hipMalloc very often returns zeroed pages, so a
kernel that reads a word it never wrote -- a count, a flag, a histogram bin, a list length -- passes on a fresh arena and after its own
previous call, and breaks only behind another family.  Here every user runs behind every other user (b), on arenas filled with 0x00,
0xFF and 0xA5 through pvf_debug_scratch (c), and small after large (d); (a) holds the sharing table against the library, so that a
verb moved to another arena fails until somebody has re-read who shares it; (f) tests the debug entry itself.  Every step compares with
the verb's own reference under the verb's own equality (scratch_cases.py); no tolerance is introduced here.

Contexts are opened per test and closed in `finally`; the session context only computes the reference matrices of the agglomeration.
All ordered pairs of every shared arena run (72, 42, 30, 20, 6 and 2): none is left out."""
import ctypes as C

import numpy as np
import pytest

from tests import scratch_cases as sc

pytestmark = pytest.mark.gpu

SMALL_LARGE_SMALL = [u for u in sc.USERS if any(u in sc.SHARERS[a] for a in ("s_act0", "s_trk0", "s_clu0", "s_clu1"))]
_FRESH = {}


@pytest.fixture(scope="module", autouse=True)
def configured(model_paths, ctx):
    sc.configure(model_paths, ctx)


def fresh_small(user):
    """{arena: bytes} after `user`'s small step on a fresh context: what that step needs, with DevBuf's slack"""
    if user not in _FRESH:
        c = sc.open_context(sc.kinds_of(user))
        try:
            sc.step(user, "small")(c)
            _FRESH[user] = c.scratch()
        finally:
            c.close()
    return _FRESH[user]


def need_of(cap):
    """the bytes a call asked DevBuf::ensure for when the buffer it got holds `cap` (n + n / 8 + 256, csrc/pvf_internal.h)"""
    n = max(0, (cap - 256) * 8 // 9 - 2)
    while n + n // 8 + 256 < cap:
        n += 1
    assert n + n // 8 + 256 == cap, cap
    return n


def same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- a. the table is the code's -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("user", list(sc.USERS))
def test_the_table_names_the_arenas_a_user_grows(user):
    c = sc.open_context(sc.kinds_of(user))
    try:
        before, held = c.scratch(state=True)
        assert set(sc.SHARERS) <= set(before) and held == {"s_feat", "s_orb_set"}
        assert all(before[a] == 0 for a in before if a not in held), before          # a fresh context has carved nothing
        sc.step(user, "small")(c)
        after = c.scratch()
    finally:
        c.close()
    _FRESH.setdefault(user, after)
    grown = {a for a in after if after[a] > before[a]}
    listed = set(sc.arenas_of(user))
    assert listed <= grown, ("the table lists arenas the user does not touch", sorted(listed - grown))
    assert not (grown - listed - held), ("the user grows call-local arenas the table does not list for it", sorted(grown - listed - held))


# ---- b. every sharer behind every other -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arenas", sc.SHARED, ids=["+".join(a) for a in sc.SHARED])
def test_every_sharer_behind_every_other(arenas):
    users = sc.SHARERS[arenas[0]]
    assert all(sc.SHARERS[a] == users for a in arenas)
    bad, pairs = [], 0
    for V in users:
        for U in users:
            if U == V:
                continue
            pairs += 1
            c = sc.open_context(sc.kinds_of(U, V))
            try:
                for who, size in ((V, "large"), (U, "small"), (V, "small"), (U, "large")):
                    before = c.scratch()
                    try:
                        sc.step(who, size)(c)
                    except AssertionError as e:
                        bad.append((V, U, "%s %s" % (who, size), str(e)[:400]))
                    after = c.scratch()
                    for a in arenas:
                        # the large step must leave more than the small one behind it takes on its own, and the small one must then have
                        # run inside that buffer: otherwise the pair proves nothing
                        if (who, size) == (V, "large") and after[a] <= need_of(fresh_small(U)[a]):
                            bad.append((V, U, "%s large leaves %s at %d bytes, %s small asks for %d" % (V, a, after[a], U, need_of(fresh_small(U)[a]))))
                        if (who, size) == (U, "small") and after[a] != before[a]:
                            bad.append((V, U, "%s small regrew %s from %d to %d bytes" % (U, a, before[a], after[a])))
            finally:
                c.close()
    assert pairs == len(users) * (len(users) - 1)
    assert not bad, (len(bad), bad[:20])


# ---- c. poisoned memory ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", sc.FILLS, ids=["0x%02X" % f for f in sc.FILLS])
@pytest.mark.parametrize("user", list(sc.USERS))
def test_on_poisoned_arenas(user, fill, monkeypatch):
    u = sc.USERS[user]
    small, large = sc.step(user, "small"), sc.step(user, "large")
    c = sc.open_context(sc.kinds_of(user))
    try:
        clean_large, clean_small = large(c), small(c)                # (each compared with its reference; the arenas are grown now)
        grown = c.scratch()
        for rounds in ({}, u.rounds) if u.rounds else ({},):
            for k, v in rounds.items():
                monkeypatch.setenv(k, v)
            c.scratch(fill)
            s = small(c)
            c.scratch(fill)
            l = large(c)
            if u.exact:
                assert same_bits(s, clean_small), (user, fill, rounds, "the small step's bits moved with what lay in the arenas")
                assert same_bits(l, clean_large), (user, fill, rounds, "the large step's bits moved with what lay in the arenas")
        assert c.scratch() == grown                                  # nothing grew: every step ran on the filled bytes
    finally:
        c.close()


# ---- d. small, large, small -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("user", SMALL_LARGE_SMALL)
def test_small_large_small(user):
    small, large = sc.step(user, "small"), sc.step(user, "large")
    c = sc.open_context(sc.kinds_of(user))
    try:
        first = small(c)
        large(c)
        grown = c.scratch()
        third = small(c)                                             # on a buffer far larger than its layout, full of the second call's data
        assert c.scratch() == grown
    finally:
        c.close()
    for a in sc.arenas_of(user):
        assert grown[a] >= fresh_small(user)[a], a
    assert any(grown[a] > fresh_small(user)[a] for a in sc.arenas_of(user))
    if sc.USERS[user].exact:
        assert same_bits(third, first)


# ---- f. the entry itself --------------------------------------------------------------------------------------------------------------
def test_a_refused_fill_writes_nothing():
    from pyannote_video_amd import _lib
    c = sc.open_context()
    try:
        first = sc.step("clothes", "small")(c)                       # (its histogram rows lie in s_act0: a fill would show in an unzeroed bin)
        sc.step("runs", "large")(c)
        before = c.scratch(state=True)
        report = np.full(4096, 0xA5, np.uint8)
        need = C.c_int64(-7)
        for fill in (-2, 256, 1 << 20, -(1 << 31)):
            with pytest.raises(_lib.PvfError, match="fill is a byte 0..255, or -1"):
                c.scratch(fill)
            assert c._l.pvf_debug_scratch(c._h, fill, _lib.ptr(report), report.nbytes, C.byref(need)) != 0
            assert need.value == -7 and (report == 0xA5).all()       # refused before any work: nothing reported either
            assert c.scratch(state=True) == before
            assert same_bits(sc.step("clothes", "small")(c), first)  # the context goes on, and the step is still exact
        assert c._l.pvf_debug_scratch(c._h, -1, None, 0, None) != 0 and b"pvf_debug_scratch" in c._l.pvf_last_error()
        assert c._l.pvf_debug_scratch(c._h, -1, None, 8, C.byref(need)) != 0 and need.value == -7
        assert c.scratch(state=True) == before
    finally:
        c.close()


def test_a_report_buffer_that_is_too_small():
    from pyannote_video_amd import _lib
    c = sc.open_context()
    try:
        sc.step("search", "large")(c)
        need = C.c_int64(0)
        assert c._l.pvf_debug_scratch(c._h, -1, None, 0, C.byref(need)) == 0 and need.value > 100
        n = need.value
        for cap in (0, 1, n - 1):                                    # too small: the size comes back, nothing is written
            buf = np.full(n + 8, 0xA5, np.uint8)
            need.value = 0
            assert c._l.pvf_debug_scratch(c._h, -1, _lib.ptr(buf), cap, C.byref(need)) == 0
            assert need.value == n and (buf == 0xA5).all(), cap
        buf = np.full(n + 8, 0xA5, np.uint8)                         # exactly enough: the text with its NUL, the guard behind it untouched
        assert c._l.pvf_debug_scratch(c._h, -1, _lib.ptr(buf), n, C.byref(need)) == 0 and need.value == n
        assert buf[n - 1] == 0 and (buf[:n - 1] != 0).all() and (buf[n:] == 0xA5).all()
        lines = buf[:n - 1].tobytes().decode().splitlines()
        assert [l.split()[0] for l in lines] == list(c.scratch()) and all(len(l.split()) in (2, 3) for l in lines)
        assert {l.split()[0]: int(l.split()[1]) for l in lines} == c.scratch()
        assert [l.split()[0] for l in lines if l.endswith(" state")] == ["s_feat", "s_orb_set"]
    finally:
        c.close()


def test_a_fill_leaves_the_arenas_that_hold_state_alone():
    """s_feat keeps the zero border of the detector's feature maps (written once per plan), s_orb_set the resident descriptor sets: a
    detector call of the same plan and the matcher on the resident sets give after a fill what they gave before it"""
    import detector_cases as dc
    g = dc.by_name("40x40_up0")
    c = sc.open_context()
    try:
        with sc._uploaded(c, [dc.case_frame(g, "noise")]) as devs:
            raw = c.detect_raw(devs[0], g.up, dc.ALL_PASS)
            assert len(raw) == g.pairs                               # every window of every level
            sc.step("orb", "large")(c)
            pairs, want = sc._orb_case("large")[5:7]
            assert min(want) > 0 and np.array_equal(c.orb_match_counts(pairs), want)
            before, held = c.scratch(state=True)
            assert before["s_feat"] > 0 and before["s_orb_set"] > 0 and before["s_pyr"] > 0
            for fill in (0xFF, 0xA5):
                assert c.scratch(fill) == before
                assert np.array_equal(c.orb_match_counts(pairs), want), fill
                assert c.detect_raw(devs[0], g.up, dc.ALL_PASS) == raw, fill
    finally:
        c.close()
