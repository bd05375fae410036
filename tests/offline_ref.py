"""Whole-file diarization in float64 numpy: the yardstick of tests/test_offline_host.py and tests/test_gpu_offline.py.

It states the definition directly and shares nothing with the package: the linkage keeps every cluster's CENTROID (the
plain mean of its members' unit rows) and measures distances between centroids, where the library updates a matrix of
squared distances by the Lance-Williams formula; the cut walks the tree; the reconstruction is array statements.  Each
stage also reports its MARGIN, the distance of the input from a decision that rounding could flip: the tests demand
identical decisions only of inputs whose margin is far above the rounding bound, and assert that it is."""
import math

import numpy as np


def rows_of(seg, emb, tau_active, min_clean_ratio=0.2):
    """seg (C, F, K), emb (C, K, D) -> x (R, D) float64 unit rows of the usable (c, k) in row-major order, `usable`
    (C, K) bool, `train` (N,) indices into x, `on` (C, F, K) bool, `valid` (C,) bool.  Written as the rules read, one
    (chunk, local speaker) at a time, so that it shares no array expression with the package."""
    seg = np.asarray(seg, dtype=np.float32)
    emb = np.asarray(emb, dtype=np.float32)
    C, F, K = seg.shape
    need = math.ceil(min_clean_ratio * F)
    valid = np.zeros(C, dtype=bool)
    on = np.zeros((C, F, K), dtype=bool)
    usable = np.zeros((C, K), dtype=bool)
    rows, train = [], []
    for c in range(C):
        valid[c] = all(math.isfinite(v) for v in seg[c].ravel().tolist())
        if valid[c]:
            for f in range(F):
                for k in range(K):
                    on[c, f, k] = float(seg[c, f, k]) > float(tau_active)
        for k in range(K):
            e = emb[c, k].astype(np.float64)
            if not all(math.isfinite(v) for v in e.tolist()):
                continue
            norm = math.sqrt(float((e * e).sum()))
            frames_on = [f for f in range(F) if on[c, f, k]]
            if not math.isfinite(norm) or norm == 0.0 or len(frames_on) < 1:
                continue
            clean = [f for f in frames_on if sum(bool(on[c, f, j]) for j in range(K)) == 1]
            usable[c, k] = True
            if len(clean) >= need:
                train.append(len(rows))
            rows.append(e / norm)
    x = np.stack(rows) if rows else np.zeros((0, emb.shape[2]))
    return x, usable, np.array(train, dtype=np.int64), on, valid


def linkage(x):
    """Centroid linkage of the rows of x: Z (n - 1, 4) in scipy's layout, and per merge the gap between the chosen
    distance and the runner-up (inf for the last merge)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    Z, gaps = np.zeros((max(n - 1, 0), 4)), np.full(max(n - 1, 0), np.inf)
    if n < 2:
        return Z, gaps
    total, size, ids = x.copy(), np.ones(n, dtype=np.int64), np.arange(n)     # total: the sum of the members' rows
    M = np.full((n, n), np.inf)                                              # M[a, b], a < b: centroid distance
    for a in range(n - 1):
        M[a, a + 1:] = np.sqrt(((x[a + 1:] - x[a]) ** 2).sum(axis=1))
    alive = np.ones(n, dtype=bool)
    for t in range(n - 1):
        a, b = divmod(int(np.argmin(M)), n)
        h = M[a, b]
        M[a, b] = np.inf
        gaps[t] = M.min() - h
        Z[t] = (min(ids[a], ids[b]), max(ids[a], ids[b]), h, size[a] + size[b])
        total[b] += total[a]
        size[b] += size[a]
        ids[b] = n + t
        alive[a] = False
        M[a, :] = np.inf
        M[:, a] = np.inf
        centroid = total[b] / size[b]
        others = np.flatnonzero(alive)
        others = others[others != b]
        d = np.sqrt(((total[others] / size[others][:, None] - centroid) ** 2).sum(axis=1))
        lo, hi = others < b, others > b
        M[others[lo], b] = d[lo]
        M[b, others[hi]] = d[hi]
    return Z, gaps


def linkage_fast(x):
    """The same Z and gaps as `linkage` (tests/test_offline_host.py holds the two against each other), for sizes at which
    a pass over the whole matrix per merge takes too long: the lowest distance of every row is kept, a row is scanned
    again when the cluster it named merged, and the runner-up is the lower of the winning row's second entry and the
    other rows' lowest.  Distances are still measured between centroids."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    Z, gaps = np.zeros((max(n - 1, 0), 4)), np.full(max(n - 1, 0), np.inf)
    if n < 2:
        return Z, gaps
    total, size, ids = x.copy(), np.ones(n, dtype=np.int64), np.arange(n)
    M = np.full((n, n), np.inf)
    for a in range(n - 1):
        M[a, a + 1:] = np.sqrt(((x[a + 1:] - x[a]) ** 2).sum(axis=1))
    low, arg = M.min(axis=1), M.argmin(axis=1)
    alive = np.ones(n, dtype=bool)
    for t in range(n - 1):
        a = int(np.argmin(low))                  # the first row among equal lows, its first column among equal entries:
        b = int(arg[a])                          # the entry argmin of the flattened matrix finds
        h = M[a, b]
        M[a, b] = np.inf
        low[a] = np.inf
        gaps[t] = min(M[a].min(), low.min()) - h
        Z[t] = (min(ids[a], ids[b]), max(ids[a], ids[b]), h, size[a] + size[b])
        total[b] += total[a]
        size[b] += size[a]
        ids[b] = n + t
        alive[a] = False
        M[a, :] = np.inf
        M[:, a] = np.inf
        centroid = total[b] / size[b]
        others = np.flatnonzero(alive)
        others = others[others != b]
        d = np.sqrt(((total[others] / size[others][:, None] - centroid) ** 2).sum(axis=1))
        lo, hi = others < b, others > b
        M[others[lo], b] = d[lo]
        M[b, others[hi]] = d[hi]
        again = np.flatnonzero(alive & ((arg == a) | (arg == b)))
        again = np.union1d(again, [b])
        low[again], arg[again] = M[again].min(axis=1), M[again].argmin(axis=1)
        better = others[lo][(d[lo] < low[others[lo]]) | ((d[lo] == low[others[lo]]) & (b < arg[others[lo]]))]
        low[better], arg[better] = M[better, b], b
    return Z, gaps


def height_bound(Z):
    """The tolerance of each height: 32 N 2^-52 / max(h, 1e-3)."""
    n = Z.shape[0] + 1
    return 32.0 * n * 2.0 ** -52 / np.maximum(Z[:, 2], 1e-3)


def flat_clusters(Z, n, threshold):
    """fcluster(Z, threshold, "distance"): a flat cluster is a maximal subtree whose merge heights are all <= threshold.
    Returns one arbitrary label per leaf."""
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    top = np.zeros(2 * n - 1)
    kids = {}
    for t in range(n - 1):
        a, b = int(Z[t, 0]), int(Z[t, 1])
        kids[n + t] = (a, b)
        top[n + t] = max(Z[t, 2], top[a], top[b])
    labels, todo, count = np.full(n, -1, dtype=np.int64), [(2 * n - 2, -1)], 0
    while todo:
        node, c = todo.pop()
        if c < 0 and (node < n or top[node] <= threshold):
            c, count = count, count + 1
        if node < n:
            labels[node] = c
        else:
            todo += [(kids[node][0], c), (kids[node][1], c)]
    return labels


def keep_clusters(flat, min_cluster_size, max_speakers):
    """flat labels -> per leaf the kept cluster 0 .. G - 1 (numbered by first member) or -1, and G."""
    n = flat.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int64), 0
    names = np.unique(flat)
    members = {c: np.flatnonzero(flat == c) for c in names}
    ranked = sorted(names, key=lambda c: (-members[c].shape[0], members[c][0]))
    kept = [c for c in ranked if members[c].shape[0] >= min_cluster_size][:max_speakers] or [ranked[0]]
    kept.sort(key=lambda c: members[c][0])
    out = np.full(n, -1, dtype=np.int64)
    for g, c in enumerate(kept):
        out[members[c]] = g
    return out, len(kept)


def cluster(x, train, threshold, min_cluster_size=12, max_speakers=20):
    """x (R, D) usable unit rows, train their clustered subset -> assign (R,), G, and the margins (merge gaps over their
    bounds, the heights' distance from the threshold, the assignment's best-to-second gap)."""
    R = x.shape[0]
    info = dict(merge_ratio=np.inf, threshold_gap=np.inf, assign_gap=np.inf, Z=np.zeros((0, 4)))
    if R == 0:
        return np.zeros(0, dtype=np.int64), 0, info
    if train.shape[0] == 0:
        return np.zeros(R, dtype=np.int64), 1, info           # all usable rows form one cluster
    Z, gaps = linkage(x[train])
    info["Z"] = Z
    if Z.shape[0]:
        info["merge_ratio"] = float((gaps / height_bound(Z)).min())
        info["threshold_gap"] = float(np.abs(Z[:, 2] - threshold).min())
    labels, G = keep_clusters(flat_clusters(Z, train.shape[0], threshold), min_cluster_size, max_speakers)
    centroids = np.stack([x[train[labels == g]].mean(axis=0) for g in range(G)])
    dist = 1.0 - (x @ centroids.T) / np.sqrt((centroids * centroids).sum(axis=1))[None, :]
    assign = np.argmin(dist, axis=1)
    if G > 1:
        two = np.sort(dist, axis=1)[:, :2]
        info["assign_gap"] = float((two[:, 1] - two[:, 0]).min())
    return assign, G, info


def reconstruct(seg, assign_ck, on, valid, starts, res, G):
    """-> active (T, G) bool.  assign_ck (C, K): the cluster of each local speaker or -1."""
    seg = np.asarray(seg, dtype=np.float64)
    C, F, K = seg.shape
    offs = np.rint((np.asarray(starts, dtype=np.float64) - starts[0]) / res).astype(np.int64)
    T = int(offs[-1]) + F
    A, on_sum, cover = np.zeros((T, G)), np.zeros(T), np.zeros(T)
    for c in range(C):
        if not valid[c]:
            continue
        a = np.zeros((F, G))
        for g in range(G):
            ks = np.flatnonzero(assign_ck[c] == g)
            if ks.size:
                a[:, g] = seg[c][:, ks].max(axis=1)
        A[offs[c]:offs[c] + F] += a
        on_sum[offs[c]:offs[c] + F] += on[c].sum(axis=1)
        cover[offs[c]:offs[c] + F] += 1
    count = np.zeros(T, dtype=np.int64)
    covered = cover > 0
    count[covered] = np.minimum(np.rint(on_sum[covered] / cover[covered]), G).astype(np.int64)
    order = np.argsort(-A, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(G), (T, G)), axis=1)
    return (rank < count[:, None]) & (A > 0), dict(A=A, mean=np.where(covered, on_sum / np.maximum(cover, 1), 0.0))


def turns(active, starts, res, shift):
    """-> sorted [(start, end, label)] with frame middles as the turn boundaries."""
    t0 = float(starts[0]) + float(shift)
    out = []
    for g in range(active.shape[1]):
        on = np.concatenate([[False], active[:, g], [False]])
        edges = np.flatnonzero(on[1:] != on[:-1])
        out += [(t0 + (s + 0.5) * res, t0 + (e + 0.5) * res, f"speaker{g}") for s, e in zip(edges[::2], edges[1::2])]
    return sorted(out)


def diarize(seg, emb, starts, res, shift, threshold, tau_active, min_clean_ratio=0.2, min_cluster_size=12, max_speakers=20):
    """One file, end to end -> (turns, info); info carries the margins, the assignment (C, K) and `active`."""
    x, usable, train, on, valid = rows_of(seg, emb, tau_active, min_clean_ratio)
    assign, G, info = cluster(x, train, threshold, min_cluster_size, max_speakers)
    assign_ck = np.full(usable.shape, -1, dtype=np.int64)
    assign_ck[usable] = assign
    info.update(assign=assign_ck, G=G, x=x, train=train)
    if G == 0:
        info["active"] = np.zeros((0, 0), dtype=bool)
        return [], info
    active, extra = reconstruct(seg, assign_ck, on, valid, starts, res, G)
    info.update(active=active, **extra)
    return turns(active, starts, res, shift), info


def clustered_rows(rng, n, dim, clusters, noise):
    """n unit rows around `clusters` random unit centres with Gaussian noise: the generator of the linkage cases."""
    centres = rng.standard_normal((clusters, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[rng.integers(0, clusters, n)] + noise * rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def is_dendrogram(Z, n):
    """Every node is merged exactly once, sizes add up, ids are ordered, heights are finite and non-negative."""
    if Z.shape != (max(n - 1, 0), 4):
        return False
    size = {i: 1 for i in range(n)}
    for t in range(n - 1):
        a, b = Z[t, 0], Z[t, 1]
        if a != int(a) or b != int(b) or not a < b or int(a) not in size or int(b) not in size:
            return False
        merged = size.pop(int(a)) + size.pop(int(b))
        if Z[t, 3] != merged or not np.isfinite(Z[t, 2]) or Z[t, 2] < 0:
            return False
        size[n + t] = merged
    return len(size) == (1 if n else 0)
