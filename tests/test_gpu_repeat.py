"""GPU: the `fingerprint` and `repeat` verbs' kernels (csrc/repeat.hip) against REPEAT.md as tests/repeat_ref.py restates it, with
np.array_equal: the prints over frame sizes, contents, batches and sources; the runs over the table sizes, seams, thresholds and modes
of tests/repeat_cases.py (whose reach tests/test_repeat_ref.py proves on the CPU); the overflow protocol; every refusal; and the two
verbs in processes of their own."""
import ctypes
import json
import os
import subprocess
import sys

import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships
import numpy as np
import pytest

from tests import repeat_cases as rc, repeat_ref as rr
from tests.test_gpu_faces import bare_ctx      # noqa: F401 -- fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = rc.S


def _same(got, want, what=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d differ, first at %s: %s against %s" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- prints -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", rc.SIZES)
def test_prints_of_every_content_at_one_size(bare_ctx, w, h):
    frames = [rc.make_frame(w, h, c) for c in rc.CONTENTS] + [rc.make_frame(w, h, "noise", seed=s) for s in (1, 2)]
    devs = [bare_ctx.upload(f) for f in frames]
    got = bare_ctx.frame_prints(devs)
    again = bare_ctx.frame_prints(devs)                             # the same call twice
    for d in devs:
        d.release()
    _same(got, rr.prints(frames), (w, h))
    _same(again, got)


def test_print_of_one_2160p_frame(bare_ctx):
    w, h = rc.BIG_SIZE
    f = rc.make_frame(w, h, "noise")
    f[: h // 3, : w // 2] |= 0xC0                # not all of it averages to 127
    dev = bare_ctx.upload(f)
    got = bare_ctx.frame_prints([dev])
    dev.release()
    _same(got, rr.prints([f]))
    assert rr.range_of(got)[0] > 16


def test_mixed_sizes_batches_and_where_the_output_lies(bare_ctx):
    from pyannote_video_amd import _lib
    sizes = [(1, 1), (7, 10), (64, 36), (9, 9), (33, 21), (8, 8), (130, 3), (3, 130), (641, 359)]
    frames = [rc.make_frame(w, h, "noise", seed=k) for k, (w, h) in enumerate(sizes * 3)]
    want = rr.prints(frames)
    devs = [bare_ctx.upload(f) for f in frames]
    for n in (1, 2, len(frames)):
        _same(bare_ctx.frame_prints(devs[:n]), want[:n], n)
    assert bare_ctx.frame_prints([]).shape == (0, 4)
    hs = np.array([d.handle for d in devs[:5]], np.uint64)
    buf = np.full(5 * 4 + 2, 0xA5A5A5A5, np.uint64)                 # host memory, the words around it untouched
    assert bare_ctx._l.pvf_frame_prints(bare_ctx._h, _lib.ptr(hs), 5, buf[1:].ctypes.data, 0) == 0
    assert np.array_equal(buf[1:21].reshape(5, 4), want[:5]) and buf[0] == 0xA5A5A5A5 and buf[21] == 0xA5A5A5A5
    dev = torch.full((5 * 4 + 2,), 0x5A, dtype=torch.int64, device="cuda")      # device memory
    torch.cuda.synchronize()
    assert bare_ctx.frame_prints(devs[:5], out_ptr=dev.data_ptr() + 8) is None
    back = dev.cpu().numpy().view(np.uint64)
    assert np.array_equal(back[1:21].reshape(5, 4), want[:5]) and back[0] == 0x5A and back[21] == 0x5A
    for d in devs:
        d.release()


def test_prints_of_frames_from_the_rings(bare_ctx):
    from pyannote_video_amd.y4m import YuvFrame
    from tests import yuv_ref
    h, w = 54, 96
    clip = [rc.make_frame(w, h, "noise", seed=70 + i) for i in range(6)]
    ring = bare_ctx.ingest_ring(h, w, depth=4)
    devs = [ring.push(f) for f in clip]                             # uploads still in flight: the call waits for every frame's event
    got = bare_ctx.frame_prints(devs)
    ring.close()
    _same(got, rr.prints(clip), "rgb ring")
    for d in devs:
        d.release()
    planes = [yuv_ref.noise_planes(h, w, "420", 90 + i) for i in range(6)]
    yring = bare_ctx.ingest_ring_yuv(h, w, layout="420", depth=4)
    devs = [yring.push(YuvFrame(*p)) for p in planes]
    got = bare_ctx.frame_prints(devs)
    yring.close()
    _same(got, rr.prints([yuv_ref.to_rgb(*p) for p in planes]), "yuv ring")
    for d in devs:
        d.release()


# ---- runs ---------------------------------------------------------------------------------------------------------------------------
def both(ctx, case, **kw):
    """the library's runs of a case and the restatement's"""
    got = ctx.print_runs(case.A, case.ua, case.B, case.ub, **kw)
    want = rr.runs(case.A, case.ua, case.B, case.ub, strip=S, **kw)
    _same(got, want, (case.name, kw))
    return got


@pytest.mark.parametrize("NA,NB", rc.SIZE_PAIRS + rc.THIN)
def test_table_sizes(bare_ctx, NA, NB):
    case = rc.size_case(NA, NB)
    n = min(NA, NB, 5)
    got = both(bare_ctx, case, tau=rc.TAU_RANDOM)
    assert got.tolist() == [[NA - n, NB - n, n]]
    for L in sorted(set((1, min(NA, NB, 4), min(NA, NB)))):         # every pair matches: NA + NB - 1 - 2 (L - 1) runs
        assert len(both(bare_ctx, case, tau=128, min_len=L)) == rr.run_count_all_match(NA, NB, L)


@pytest.fixture(scope="module")
def seams():
    return rc.seam_case()


@pytest.mark.parametrize("tau", [0, rc.PLANT_BITS - 1, rc.PLANT_BITS, rc.TAU_RANDOM])
def test_planted_runs_at_every_seam(bare_ctx, seams, tau):
    got = both(bare_ctx, seams, tau=tau)
    want = sorted(((p.i, p.j, p.n) for p in seams.plants if p.bits <= tau), key=lambda r: (r[1] - r[0], r[0]))
    assert got.tolist() == [list(r) for r in want]
    again = bare_ctx.print_runs(seams.A, seams.ua, seams.B, seams.ub, tau=tau)          # the same call twice
    _same(again, got)


def test_every_pair_matches_over_three_strips(bare_ctx, seams):
    got = both(bare_ctx, seams, tau=128, min_len=3)
    assert len(got) == rr.run_count_all_match(rc.SEAM_NA, rc.SEAM_NB, 3)


def test_min_len_at_a_runs_length_and_one_above(bare_ctx, seams):
    for L in (4, 5, 6, 7, 8, 11, 2 * S + 10, 2 * S + 11):
        got = both(bare_ctx, seams, tau=rc.PLANT_BITS, min_len=L)
        assert len(got) == sum(1 for p in seams.plants if p.n >= L)


def test_usable_bytes_cut_runs(bare_ctx, seams):
    long = [p for p in seams.plants if p.n > 2 * S][0]
    one = [p for p in seams.plants if p.what == "crosses one seam"][0]
    ua, ub = seams.ua.copy(), seams.ub.copy()
    assert one.i + 4 == 2 * S - 1 == long.i + S + 2
    ua[2 * S - 1] = 0                            # the last row of a strip, on A's side: it lies in both runs
    ub[long.j + S + 3] = 0                       # the long run's cell on the first row of the next strip, on B's side
    cut = seams._replace(ua=ua, ub=ub)
    got = both(bare_ctx, cut, tau=rc.PLANT_BITS)
    rows = got.tolist()
    assert [long.i, long.j, S + 2] in rows and [long.i + S + 4, long.j + S + 4, long.n - S - 4] in rows
    assert [one.i, one.j, 4] in rows and [one.i + 5, one.j + 5, one.n - 5] in rows
    assert len(got) == len(seams.plants) + 2
    both(bare_ctx, cut, tau=128, min_len=2)
    none = seams._replace(ua=np.zeros_like(ua))
    assert len(both(bare_ctx, none, tau=128)) == 0
    none = seams._replace(ub=np.zeros_like(ub))
    assert len(both(bare_ctx, none, tau=128)) == 0


def test_all_equal_prints_every_diagonal_is_one_run(bare_ctx):
    case = rc.all_equal(600, 600)
    got = both(bare_ctx, case, tau=0)
    assert len(got) == 1199 and got[:, 2].max() == 600
    case = rc.all_equal(S + 40, 2 * S + 3)       # the walk past the strip is most of the work
    got = both(bare_ctx, case, tau=0, min_len=S)
    assert len(got) == rr.run_count_all_match(S + 40, 2 * S + 3, S)


def test_self_mode(bare_ctx):
    case = rc.self_case()
    N = len(case.A)
    got = both(bare_ctx, case, tau=rc.PLANT_BITS, min_gap=1)
    want = sorted(((p.i, p.j, p.n) for p in case.plants), key=lambda r: (r[1] - r[0], r[0]))
    assert got.tolist() == [list(r) for r in want]
    got = both(bare_ctx, case, tau=rc.PLANT_BITS, min_gap=2)
    assert len(got) == len(want) - 1 and [50, 51, 7] not in got.tolist()
    for g in (1, 2, 3, N - 2, N - 1):            # every pair matches: diagonal g .. N - 1, a run each
        assert len(both(bare_ctx, case, tau=128, min_gap=g)) == N - g
    assert both(bare_ctx, case, tau=128, min_gap=N - 1).tolist() == [[0, N - 1, 1]]
    assert len(both(bare_ctx, case, tau=128, min_gap=N)) == 0
    assert len(both(bare_ctx, case, tau=128, min_gap=N + 5)) == 0
    tiny = rc.RunCase("tiny", case.A[:1], case.ua[:1], None, None, ())
    assert len(both(bare_ctx, tiny, tau=128, min_gap=1)) == 0


def raw_call(ctx, case, tau0, cap0, **over):
    """pvf_print_runs on a case, with any argument replaced -> (return code, found, the run buffer with a guard row behind cap)"""
    from pyannote_video_amd import _lib
    P = _lib.ptr
    runs = np.full((max(cap0, 0) + 1, 3), -7, np.int32)
    found = ctypes.c_int64(-1)
    a = dict(A=P(case.A), ua=P(case.ua), NA=len(case.A), B=P(case.B) if case.B is not None else None,
             ub=P(case.ub) if case.ub is not None else None, NB=len(case.B) if case.B is not None else 0, tau=tau0, min_len=1, min_gap=1,
             runs=P(runs), cap=cap0, found=ctypes.byref(found))
    a.update(over)
    rc_ = ctx._l.pvf_print_runs(ctx._h, a["A"], a["ua"], a["NA"], a["B"], a["ub"], a["NB"], a["tau"], a["min_len"], a["min_gap"], a["runs"], a["cap"],
                                a["found"])
    return rc_, found.value, runs


def test_the_overflow_protocol(bare_ctx, seams):
    want = rr.runs(seams.A, seams.ua, seams.B, seams.ub, tau=rc.PLANT_BITS)
    n = len(want)
    code, found, runs = raw_call(bare_ctx, seams, rc.PLANT_BITS, n)
    assert code == 0 and found == n and np.array_equal(runs[:n], want) and (runs[n] == -7).all()
    for cap in (n - 1, 0):
        code, found, runs = raw_call(bare_ctx, seams, rc.PLANT_BITS, cap)
        assert code == 0 and found == n and (runs[cap] == -7).all()             # the same found; nothing behind cap is touched
        code, found, runs = raw_call(bare_ctx, seams, rc.PLANT_BITS, found)     # the second call returns the runs
        assert code == 0 and found == n and np.array_equal(runs[:n], want)
    _same(bare_ctx.print_runs(seams.A, seams.ua, seams.B, seams.ub, tau=rc.PLANT_BITS, cap=1), want)      # Context.print_runs does it itself


def test_refusals(bare_ctx):
    from pyannote_video_amd import _lib
    c, l = bare_ctx, bare_ctx._l
    case = rc.size_case(40, 30)
    want = rr.runs(case.A, case.ua, case.B, case.ub, tau=rc.TAU_RANDOM)
    big = (1 << 24) + 1
    for kw, message in ((dict(NA=-1), "PVF_PRINT_MAX_ROWS"), (dict(NA=big), "PVF_PRINT_MAX_ROWS"), (dict(NB=-1), "PVF_PRINT_MAX_ROWS"),
                        (dict(NB=big), "PVF_PRINT_MAX_ROWS"), (dict(tau=-1), "tau outside"), (dict(tau=129), "tau outside"),
                        (dict(min_len=0), "min_len below 1"), (dict(B=None, min_gap=0), "min_gap >= 1"), (dict(cap=-1), "cap below 0"),
                        (dict(found=None), "null found"), (dict(A=None), "null A or usable_a"), (dict(ua=None), "null A or usable_a"),
                        (dict(ub=None), "null usable_b"), (dict(runs=None), "null runs")):
        code, found, runs = raw_call(c, case, rc.TAU_RANDOM, 8, **kw)
        assert code != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert (runs == -7).all() and found == -1                   # refused before any work
        code, found, runs = raw_call(c, case, rc.TAU_RANDOM, 8)     # the context goes on
        assert code == 0 and found == len(want) and np.array_equal(runs[:found], want)
    empty = rc.RunCase("empty", case.A[:0], case.ua[:0], case.B, case.ub, ())
    assert raw_call(c, empty, 128, 4, A=None, ua=None)[:2] == (0, 0)              # a count of 0 is legal and finds nothing
    empty = rc.RunCase("empty", case.A, case.ua, case.B[:0], case.ub[:0], ())
    assert raw_call(c, empty, 128, 4)[:2] == (0, 0)
    # prints
    f = rc.make_frame(12, 7, "noise")
    a, gone = c.upload(f), c.upload(f)
    gone_handle = gone.handle
    gone.release()
    hs = np.array([a.handle, a.handle], np.uint64)
    out = np.zeros((2, 4), np.uint64)
    ref = rr.prints([f, f])

    def call(frames=hs, n=2, o=out):
        return l.pvf_frame_prints(c._h, _lib.ptr(frames) if frames is not None else None, n, _lib.ptr(o) if o is not None else None, 0)
    for kw, message in ((dict(n=-1), "PVF_PRINT_MAX_ROWS"), (dict(n=big), "PVF_PRINT_MAX_ROWS"), (dict(frames=None), "null frames or output"),
                        (dict(o=None), "null frames or output"), (dict(frames=np.array([a.handle, 987654321], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([gone_handle, a.handle], np.uint64)), "unknown frame handle")):
        assert call(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert not out.any()
        assert call() == 0 and np.array_equal(out, ref)
        out[:] = 0
    assert l.pvf_frame_prints(c._h, None, 0, None, 0) == 0
    a.release()
    with pytest.raises(ValueError, match="uint64"):
        c.print_runs(case.A.astype(np.int64), case.ua)
    with pytest.raises(ValueError, match="usable byte"):
        c.print_runs(case.A, case.ua[:-1])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_the_verbs_in_processes_of_their_own(tmp_path):
    from pyannote_video_amd import synth
    fps = 5.0
    v = synth.SyntheticVideo(width=96, height=54, n_frames=40, n_shots=4, faces=1, min_face=12, max_face=20, seed=3, frame_rate=fps)
    base = [v.frame(i) for i in range(40)]
    film_a = base[:30] + base[4:16] + base[30:34]                   # frames 4 .. 15 come again as 30 .. 41: a recap inside one film
    film_b = base[34:40] + base[2:18] + base[36:40]                 # and in another film as 6 .. 21
    pa, pb, va, vb, out = (str(tmp_path / n) for n in ("a.prints.npy", "b.prints.npy", "a.npy", "b.npy", "repeat.json"))
    np.save(va, np.stack(film_a))
    np.save(vb, np.stack(film_b))
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    syn = str(tmp_path / "syn.prints.npy")
    for args in (["fingerprint", "--batch", "7", va, pa], ["fingerprint", vb, pb],
                 ["fingerprint", "--from", "0.4", "--until", "2.0", "synthetic:96x54x20:2:1:3", syn],
                 ["repeat", "--min-duration", "1.0", "--min-separation", "2.0", out, pa, pb]):
        run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(fps)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             env=env, timeout=600)
        assert run.returncode == 0, (args, run.stderr.decode()[-2000:])
    want_a = rr.stamp(rr.prints(film_a), [i / fps for i in range(len(film_a))])
    want_b = rr.stamp(rr.prints(film_b), [i / fps for i in range(len(film_b))])
    _same(np.load(pa), want_a)
    _same(np.load(pb), want_b)
    sv = synth.SyntheticVideo(width=96, height=54, n_frames=20, n_shots=2, faces=1, seed=3, frame_rate=fps)
    got = np.load(syn)
    want = rr.stamp(rr.prints([sv.frame(i) for i in range(20)]), [i / fps for i in range(20)])[2:10]
    _same(got, want)
    found = json.load(open(out))
    assert found == rr.report([(pa, want_a), (pb, want_b)], min_duration=1.0, min_separation=2.0)
    assert any(s["a"] == pa and s["b"] == pb and s["offset"] == 4 and s["frames"] >= 12 for s in found), found
    assert any(s["a"] == pa and s["b"] == pa and s["offset"] == 26 and s["frames"] >= 12 for s in found), found
