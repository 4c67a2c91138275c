"""Measures the whole-frame feature tracker (include/isvins_frontend.h): one isv_fe_read_image_batch call per frame against the chain
of the existing public calls (track, reject, detect) with the bookkeeping on the host, on the same images in the same process.
512 sequences of 752 x 480, MAX_CNT 150, published frames in the steady state: the median of 5 frames after the first frame and two
warm-ups.  The first 8 items of every frame are compared bitwise with the chain.  Prints one JSON line; not a test.

    python scripts/fe_bench.py [--seqs 512] [--textures 16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import isvins_loader  # noqa: E402

isvins_loader.load()
from isvins_amd import detect as det, frontend as fe, reject as rej, tracker as trk  # noqa: E402

W, H, MAX_CNT, MIN_DIST, MAX_POINTS = 752, 480, 150, 30, 256
FRAMES, WARM = 8, 3                                  # frame 0 is the first frame, 1 and 2 warm up, 3 .. 7 are measured
F32, I32 = np.float32, np.int32


def run(n_seq, n_tex):
    tr = trk.Tracker(2 * n_seq, n_seq, W, H, max_points=MAX_POINTS)
    rj = rej.Rejector(tr)
    dt = det.Detector(tr, max_points=MAX_POINTS, max_corners=MAX_CNT, min_dist=MIN_DIST)
    f = fe.FrontEnd(tr, rj, dt)
    n_tex = min(n_tex, n_seq)
    images = [[trk.analytic_image(W, H, (1.5 * fr, -1.0 * fr), 300 + q) for q in range(n_tex)] for fr in range(FRAMES)]
    # ---- the chain's host state: readImage's bookkeeping in numpy, as a caller of the stage calls has to write it ----
    pts = [np.zeros((0, 2), F32)] * n_seq
    ids, cnt = [np.zeros(0, I32)] * n_seq, [np.zeros(0, I32)] * n_seq
    pun, pim = [np.zeros((0, 2), F32)] * n_seq, [np.zeros(0, bool)] * n_seq
    n_id, prev_time = [0] * n_seq, 0.0
    chain_ms, fe_ms, fe_parts, stage_ms, same8 = [], [], [], {}, True
    for fr in range(FRAMES):
        t = 10.0 + 0.05 * fr
        imgs = [images[fr][k % n_tex] for k in range(n_seq)]
        t0 = time.perf_counter()
        if fr == 0:
            tr.track_batch([trk.TrkItem(k, imgs[k], imgs[k]) for k in range(n_seq)])
            cur, un_t = pts, pun
            prev_un_keep, in_map_keep = pun, pim
        else:
            _, arr = tr.track_batch([trk.TrkItem(k, imgs[k], None, pts[k]) for k in range(n_seq)])
            stage_ms["track"] = tr.last_ms()
            keep = [a.flags == 3 for a in arr]
            prev = [pts[k][keep[k]] for k in range(n_seq)]
            cur = [arr[k].cur_pts[keep[k]] for k in range(n_seq)]
            un_t = [arr[k].cur_un_pts[keep[k]] for k in range(n_seq)]
            ids, cnt = [ids[k][keep[k]] for k in range(n_seq)], [cnt[k][keep[k]] + 1 for k in range(n_seq)]
            prev_un_keep, in_map_keep = [pun[k][keep[k]] for k in range(n_seq)], [pim[k][keep[k]] for k in range(n_seq)]
            _, st = rj.reject_batch([rej.RejItem(W, H, prev[k], cur[k]) for k in range(n_seq)])
            stage_ms["reject"] = rj.last_ms()
            st = [s.astype(bool) for s in st]
            cur, un_t, ids, cnt, prev_un_keep, in_map_keep = ([x[k][st[k]] for k in range(n_seq)] for x in (cur, un_t, ids, cnt, prev_un_keep, in_map_keep))
        _, darr = dt.detect_batch([det.DetItem(k, cur[k], cnt[k], max(MAX_CNT - len(cur[k]), 0)) for k in range(n_seq)])
        stage_ms["detect"] = dt.last_ms()
        chain_out = []
        for k in range(n_seq):
            kept, new, nn = darr[k].kept_index, darr[k].new_pts, len(darr[k].new_pts)
            c = np.concatenate([cur[k][kept], new]).astype(F32)
            u = np.concatenate([un_t[k][kept], darr[k].new_un_pts]).astype(F32)
            i = np.concatenate([ids[k][kept], np.full(nn, -1, I32)]).astype(I32)
            tc = np.concatenate([cnt[k][kept], np.ones(nn, I32)]).astype(I32)
            pu = np.concatenate([prev_un_keep[k][kept], np.zeros((nn, 2), F32)])
            im = np.concatenate([in_map_keep[k][kept], np.zeros(nn, bool)])
            vel = np.zeros((len(c), 2), F32)
            if len(pts[k]) > 0:                       # the map is not empty (F1)
                hit = im & (i != -1)
                with np.errstate(all="ignore"):
                    vel[hit] = ((u[hit] - pu[hit]).astype(np.float64) / (t - prev_time)).astype(F32)
            born = i == -1
            i[born] = n_id[k] + np.arange(born.sum())
            n_id[k] += int(born.sum())
            msg = tc > 1
            chain_out.append(dict(feature_id=i[msg], point=np.concatenate([u[msg].astype(np.float64), np.ones((msg.sum(), 1))], axis=1), uv=c[msg], velocity=vel[msg],
                                  cur_pts=c, cur_un_pts=u, ids=i, track_cnt=tc, pts_velocity=vel))
            pts[k], ids[k], cnt[k], pun[k], pim[k] = c, i, tc, u, ~born
        prev_time = t
        t1 = time.perf_counter()
        # ---- the one call ----
        res, frames = f.read_image_batch([fe.FeItem(n_seq + k, imgs[k], t, 1) for k in range(n_seq)])
        t2 = time.perf_counter()
        assert all(r.status == 0 for r in res)
        for k in range(min(8, n_seq)):
            for name in fe.Frame.ARRAYS:
                a, b = getattr(frames[k], name), chain_out[k][name]
                same8 = same8 and a.shape == b.shape and a.tobytes() == b.astype(a.dtype).tobytes()
        if fr >= WARM:
            chain_ms.append(1e3 * (t1 - t0)); fe_ms.append(1e3 * (t2 - t1)); fe_parts.append(f.last_ms())
    med = lambda xs: float(np.median(xs))
    parts = np.median(np.array(fe_parts), axis=0).tolist()
    out = dict(sequences=n_seq, fe_call_ms=med(fe_ms), chain_ms=med(chain_ms), fe_last_ms=dict(zip(("call", "pyramids", "flow", "reject", "detect_finish", "upload"), parts)),
               stage_last_ms={k: list(v) for k, v in stage_ms.items()}, points_per_sequence=float(np.mean([r.n_points for r in res])),
               first_8_items_bitwise_equal_to_chain=bool(same8))
    f.close(); dt.close(); rj.close(); tr.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=512)
    ap.add_argument("--textures", type=int, default=16)
    a = ap.parse_args()
    big, one = run(a.seqs, a.textures), run(1, 1)
    print(json.dumps(dict(batch=big, one_sequence=one, fe_not_slower_than_chain=big["fe_call_ms"] <= big["chain_ms"])))
