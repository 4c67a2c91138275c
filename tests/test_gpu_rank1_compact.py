"""The rank-1 downdates of the landmark elimination (rank1_body, csrc/isv_rank1.h) with each output tile's landmarks COMPACTED
-- a tile wavefront multiplies only the landmarks of the pass whose panel rows are non-zero in both its row block and its column
block, in landmark order, four per v_mfma_f64_16x16x4 -- against the dense loop it replaces (ISV_R1_DENSE=1, read when a handle
is created: every landmark of the pass through every tile).

What the compacted loop leaves out are products with an exact zero, and every output element receives its non-zero products in
the dense loop's order, so the comparison is BITWISE: the solved states, the summaries' cost / radius / accept traces and the
whole marginalisation record.  (This holds iff the instruction accumulates its four k-products as an in-order chain of fused
multiply-adds: the dense loop and the compacted one put a landmark's product into different k-slots and different quads.)
Every case is also held to the CPU oracle with the tolerances of tests/test_gpu_solve.py.

Shapes: the smallest at which the loop can go wrong -- lists that are no multiple of four and a short last pass (L = 70: 64 + 6),
one landmark, tiles without any landmark (all tracks at one end of the window), tracks that end on / start at a 16-column block
boundary (6 (h + k) = 48, 6 h = 48) and a track over all frames, and every shape of the template: nt = 3 (N = 6), nt = 5 alone /
in a batch of 4 / of 300 (above the CU count: the full-batch kernels), nt = 7 as k_rank1_mfma<7, 2> and inside k_lin_gram_chain
(four tiles per wavefront), the split elimination (700 landmarks on a one-window handle: k_rank1_split + k_schur_fold) and the
free extrinsic (EX: the pseudo-frame's columns belong to every landmark)."""
import ctypes as C

import numpy as np
import pytest

from isvins_amd import backend, synth
from test_gpu_extrinsic import check_ex, perturbed
from test_gpu_solve import check_window, oracle_run

pytestmark = pytest.mark.gpu


def _raw(x):
    return bytes(C.string_at(C.addressof(x), C.sizeof(x)))


def _handles(monkeypatch, n_frames, n_vo, **kw):
    """(dense, compacted): the same handle twice, the first created under ISV_R1_DENSE=1"""
    monkeypatch.setenv("ISV_R1_DENSE", "1")
    dense = backend.Backend(n_frames, n_vo, **kw)
    monkeypatch.delenv("ISV_R1_DENSE")
    try:
        comp = backend.Backend(n_frames, n_vo, **kw)
    except Exception:
        dense.close()
        raise
    return dense, comp


def _same_bits(ga, sa, ma, gb, sb, mb, what):
    for k, (a, b) in enumerate(zip(ga, gb)):
        assert np.array_equal(a.state_vector(), b.state_vector()), (what, "state", k)
        assert np.array_equal(a.priors_vector(), b.priors_vector()), (what, "priors", k)
    for k, (a, b) in enumerate(zip(sa, sb)):
        assert a.iterations == b.iterations and a.termination == b.termination, (what, "summary", k)
        for tr in ("trace_cost", "trace_radius", "trace_accepted"):
            assert np.array_equal(np.array(getattr(a, tr)[:]), np.array(getattr(b, tr)[:])), (what, tr, k)
        assert a.initial_cost == b.initial_cost and a.final_cost == b.final_cost, (what, "cost", k)
    for k, (a, b) in enumerate(zip(ma, mb)):
        assert _raw(a) == _raw(b), (what, "marginalisation record", k)


def _dense_vs_compact(oracle, monkeypatch, ws, n_frames=11, n_vo=5, max_batch=None, max_landmarks=None, expect=None, ex=0, **check_kw):
    """solve ws on a dense and on a compacted handle: the same bits, and the compacted side on the oracle"""
    kw = dict(max_landmarks=max_landmarks or max(w.L for w in ws), max_obs=max(w.n_obs for w in ws), max_batch=max_batch or len(ws))
    if ex:
        kw["estimate_extrinsic"] = 1
    dense, comp = _handles(monkeypatch, n_frames, n_vo, **kw)
    try:
        gd = [w.clone() for w in ws]; sd, md = dense.optimize_batch(gd)
        gc = [w.clone() for w in ws]; sc, mc = comp.optimize_batch(gc)
        if expect is not None:
            expect(dense); expect(comp)
        _same_bits(gd, sd, md, gc, sc, mc, "dense / compacted")
        if ex:
            for a, b in zip(gd, gc):
                assert np.array_equal(a.para_Ex_Pose, b.para_Ex_Pose)
        for w, g, s in zip(ws, gc, sc):
            o, so, _ = oracle_run(oracle, comp.cfg, w)
            assert s.iterations > 0
            check_window(o, so, g, s, **check_kw)
            if ex:
                check_ex(o, g)
    finally:
        dense.close(); comp.close()
    return gc, sc, mc


def _tracks(w):
    return w.lm_start_frame[: w.L].astype(int), np.diff(w.lm_obs_ptr[: w.L + 1]).astype(int)


def test_partial_quads_and_a_short_last_pass(oracle, monkeypatch):
    """70 landmarks: a pass of 64 and one of 6, lists that are no multiple of four"""
    _dense_vs_compact(oracle, monkeypatch, [synth.make_window(900, n_landmarks=70)])


def test_a_single_landmark(oracle, monkeypatch):
    _dense_vs_compact(oracle, monkeypatch, [synth.make_window(901, n_landmarks=1)])


@pytest.mark.parametrize("hosts", [(0, 3), (8, 10)])
def test_tiles_without_a_landmark(oracle, monkeypatch, hosts):
    """64 tracks of two frames, all at one end of the window: at the near end (frames 0-3: columns 0-23) the tiles of blocks
    2-3 x 2-3 get an empty list and block 4 only the rhs row; at the far end (frames 8-10: columns 48-65) blocks 0-2 stay empty"""
    w = synth.make_window(902, n_landmarks=64, host_frames=hosts, max_track=2)
    h, k = _tracks(w)
    assert h.min() >= hosts[0] and (h + k).max() <= hosts[1] + 1 and (k == 2).all()
    _dense_vs_compact(oracle, monkeypatch, [w])


def test_tracks_that_end_on_and_start_at_a_block_boundary(oracle, monkeypatch):
    """hosts 6-8 with two frames each: tracks of frames 6-7 end at column 48 = 3 x 16, tracks of frames 8-9 start there"""
    w = synth.make_window(903, n_landmarks=64, host_frames=(6, 9), max_track=2)
    h, k = _tracks(w)
    assert (6 * (h + k) == 48).any() and (6 * h == 48).any()
    _dense_vs_compact(oracle, monkeypatch, [w])


def test_a_track_over_all_frames(oracle, monkeypatch):
    w = synth.make_window(904, n_landmarks=64, host_frames=(0, 1))
    h, k = _tracks(w)
    assert ((h == 0) & (k == 11)).any()
    _dense_vs_compact(oracle, monkeypatch, [w])


def test_three_tile_rows(oracle, monkeypatch):
    """N = 6: nt = 3, six tile wavefronts"""
    ws = synth.make_windows([905, 906], n_frames=6, n_vo=3, n_landmarks=70)
    _dense_vs_compact(oracle, monkeypatch, ws, 6, 3)


@pytest.mark.parametrize("batch,n_lm", [(1, 130), (4, 130), (300, 40)])
def test_batches_of_eleven_frames(oracle, monkeypatch, capfd, batch, n_lm):
    """one window, four, and 300 -- more than the compute units: a full-batch handle (one launch per stage and k_lin_gram's
    four-wavefront form, not the small-batch handles' split solve with k_lin_gram_chain)"""
    ws = synth.make_windows(range(1000, 1000 + batch), n_landmarks=n_lm)
    monkeypatch.setenv("ISV_DEBUG_PATH", "1")                     # (read when the handle is created)
    _dense_vs_compact(oracle, monkeypatch, ws)
    err = capfd.readouterr().err
    small = "chain_split=1" if batch <= 4 else "chain_split=0"
    assert err.count("isv: handle " + small) == 2, err[-2000:]


def test_eighteen_frames_two_tiles_per_wavefront(oracle, monkeypatch):
    """N = 18 / Vo = 8 (nt = 7) on a handle for 300 windows: k_rank1_mfma<7, 2>, a wavefront with two lists and two trip counts"""
    w = synth.make_window(907, n_frames=18, n_vo=8, n_landmarks=130)
    _dense_vs_compact(oracle, monkeypatch, [w], 18, 8, max_batch=300)


def test_eighteen_frames_downdates_in_the_linearising_workgroup(oracle, monkeypatch, capfd):
    """a small batch of 18-frame windows: the downdates run inside k_lin_gram_chain, four tiles per wavefront"""
    ws = synth.make_windows([908, 909, 910], n_frames=18, n_vo=8, n_landmarks=130)
    monkeypatch.setenv("ISV_DEBUG_PATH", "1")                     # (read when the handle is created)
    _dense_vs_compact(oracle, monkeypatch, ws, 18, 8)
    err = capfd.readouterr().err
    assert "r1_in_lg=1" in err and "r1_in_lg=0" not in err, err[-2000:]


def test_one_long_window_split_over_workgroups(oracle, monkeypatch):
    """700 landmarks (11 passes) on a one-window handle: k_rank1_split's groups and k_schur_fold"""
    w = synth.make_window(911, n_landmarks=700)
    def expect(b):
        assert b.last_counts()[7] > 0                                 # the split elimination ran

    _dense_vs_compact(oracle, monkeypatch, [w], expect=expect)


def test_free_extrinsic(oracle, monkeypatch):
    """EX: the pseudo-frame's columns [6 Nr, 6 N) are non-zero for every landmark"""
    _dense_vs_compact(oracle, monkeypatch, [perturbed(912, n_landmarks=70)], ex=1)


def test_a_window_alone_and_inside_a_batch_of_four(oracle, monkeypatch):
    """the compaction depends on the window's own landmarks only: the same bits alone and beside three others on one handle"""
    ws = [synth.make_window(920 + i, n_landmarks=n) for i, n in enumerate((70, 130, 7, 64))]
    b = backend.Backend(11, 5, max_landmarks=130, max_obs=max(w.n_obs for w in ws), max_batch=4)
    try:
        gb = [w.clone() for w in ws]; sb, mb = b.optimize_batch(gb)
        for k, w in enumerate(ws):
            g1 = w.clone(); s1, m1 = b.optimize(g1)
            _same_bits([g1], [s1], [m1], [gb[k]], [sb[k]], [mb[k]], "alone / in the batch")
    finally:
        b.close()
