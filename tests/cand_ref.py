"""NumPy restatement of the top-K peak rule of mq_decode_udp_topk (include/mq_hip.h), test infrastructure only.

On the raw averaged heatmap H (h, w) of one (instance, joint):

* pixel p is a *peak* iff H[p] > min_score and every in-map 8-neighbour q has H[p] > H[q], or
  H[p] == H[q] with flat index p < q (a plateau yields exactly one peak, its lowest index);
* when the map's maximum is <= max(0, min_score) there are no peaks;
* slot 0 is the first argmax of the map with its value (``get_heatmap_maximum``), whatever the map holds;
* slots 1.. are filled greedily: the highest remaining peak (lowest flat index on ties) whose Chebyshev
  distance to every peak already taken is > min_sep; an empty slot is (-1, 0).
"""
from __future__ import annotations

import numpy as np


def find_peaks(H, min_score=0.0):
    """Flat indices of the peaks of H, ascending."""
    H = np.asarray(H, dtype=np.float32)
    h, w = H.shape
    if not H.max() > max(0.0, float(min_score)):
        return []
    out = []
    for y in range(h):
        for x in range(w):
            v = H[y, x]
            if not v > np.float32(min_score):
                continue
            p = y * w + x
            ok = True
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if (dy == 0 and dx == 0) or yy < 0 or yy >= h or xx < 0 or xx >= w:
                        continue
                    q = yy * w + xx
                    u = H[yy, xx]
                    if not (v > u or (v == u and p < q)):
                        ok = False
            if ok:
                out.append(p)
    return out


def topk_peaks(H, n_cand, min_sep=3, min_score=0.0):
    """(peak (n_cand,) int32, score (n_cand,) float32) of one map."""
    H = np.asarray(H, dtype=np.float32)
    h, w = H.shape
    peak = np.full(n_cand, -1, dtype=np.int32)
    score = np.zeros(n_cand, dtype=np.float32)
    flat = H.reshape(-1)
    peak[0] = int(np.argmax(flat))
    score[0] = flat[peak[0]]
    cands = find_peaks(H, min_score)
    cands.sort(key=lambda p: (-float(flat[p]), p))
    taken = [int(peak[0])]
    k = 1
    for p in cands:
        if k >= n_cand:
            break
        y, x = divmod(p, w)
        if all(max(abs(y - t // w), abs(x - t % w)) > min_sep for t in taken):
            peak[k] = p
            score[k] = flat[p]
            taken.append(p)
            k += 1
    return peak, score


def topk_peaks_batch(hm, n_cand, min_sep=3, min_score=0.0):
    """(n, J, h, w) -> peak (n, J, n_cand) int32, score (n, J, n_cand) float32."""
    n, J = hm.shape[:2]
    peak = np.empty((n, J, n_cand), dtype=np.int32)
    score = np.empty((n, J, n_cand), dtype=np.float32)
    for i in range(n):
        for j in range(J):
            peak[i, j], score[i, j] = topk_peaks(hm[i, j], n_cand, min_sep, min_score)
    return peak, score
