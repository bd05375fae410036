// Centroid-linkage agglomerative clustering of unit rows, float64: the ONE text of its arithmetic and decisions.
// k_agglo.hip (the kernels behind dz_agglo_linkage) and agglo.cpp (dz_agglo_linkage_host, backend="core") compile it,
// so the host and the device round alike and cannot disagree at a tie.  DESIGN.md 4.24.
//
// The state of one file of n rows lives in n SLOTS:
//   mat     (n, n)  squared Euclidean distances between the centroids of the slots' clusters, both halves kept
//   active  (n)     1 while the slot holds a cluster
//   id      (n)     the slot's scipy id: 0 .. n - 1 for the singletons, n + t for the cluster merge t made
//   size    (n)     members of the slot's cluster
//   nn_val / nn_idx (n)   the nearest active slot ABOVE the slot (m > k), lowest m among equal distances;
//                         +inf / -1 when there is none
//   stale   (n)     1: nn_val is only a lower bound of that distance (and nn_idx means nothing)
// A merge looks for the lowest (nn_val, i); while that row is stale it is scanned again and the search repeats, so
// the pair (i, j = nn_idx[i]) a merge takes is the lowest (distance, i, j) of all active pairs, exactly.  It writes
// Z[t], puts the merged cluster into slot j (the Lance-Williams centroid update of row and column j on squared
// distances, as scipy's linkage does), retires slot i, scans row j and repairs the rows below j with ag_repair.
// Centroid linkage is not reducible -- the new distance can undercut a row's current nearest -- and ag_repair's
// compare is where that is handled.  Scanning a row only when it reaches the top keeps rows that all name one growing
// cluster (random rows do: its centroid shrinks towards the origin) from being scanned at every merge.
#pragma once
#include <math.h>

#pragma clang fp contract(off)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AG_HD __host__ __device__ inline
#else
#define AG_HD inline
#endif

constexpr int AG_DMAX = 1024;            // dimension of a row
constexpr int AG_NONE = 0x7fffffff;      // "no candidate yet" index of a running minimum: loses every tie
constexpr int AG_OK = -1;                // status of a file: -1, or the merge at which an index failed its range check

// one term of the squared distance of two rows; the rows' terms are added in ascending k, by every caller
AG_HD double ag_d2_term(double s, double a, double b) {
    const double t = a - b;
    return s + t * t;
}

// the running minimum of (value, index) pairs: lower value, then lower index
AG_HD bool ag_better(double v, int idx, double best, int best_idx) { return v < best || (v == best && idx < best_idx); }
AG_HD void ag_take(double v, int idx, double& best, int& best_idx) {
    if (ag_better(v, idx, best, best_idx)) {
        best = v;
        best_idx = idx;
    }
}

// Lance-Williams, centroid linkage, on squared distances: clusters i (ni members) and j (nj) at squared distance dij
// merge; dki / dkj are cluster k's squared distances to them.  A result below 0 is taken as 0.
AG_HD double ag_lance_williams(double dki, double dkj, double dij, int ni, int nj) {
    const double a = (double)ni, b = (double)nj, n = a + b;
    const double v = (a * dki + b * dkj) / n - (a * b * dij) / (n * n);
    return v < 0.0 ? 0.0 : v;
}

// Z[t] of scipy's linkage: (smaller id, larger id, height, size)
AG_HD void ag_z_row(double* z, int id_a, int id_b, double d2, int size) {
    z[0] = (double)(id_a < id_b ? id_a : id_b);
    z[1] = (double)(id_a < id_b ? id_b : id_a);
    z[2] = sqrt(d2 < 0.0 ? 0.0 : d2);
    z[3] = (double)size;
}

// The pair a merge takes, from the lowest (nn_val, i) and what slot i names: range-checked before anything is indexed
// with it.  n slots.
AG_HD bool ag_pair_ok(int i, int j, double d2, int n, const int* active) {
    return i >= 0 && i < n && j > i && j < n && d2 == d2 && d2 < INFINITY && active[i] && active[j];
}

// Row k < j after slots i and j merged into j at squared distance nd from k.  The row's entry stays EXACT where one
// compare can keep it so: its neighbour was neither of the pair, or the merged cluster is at least as near as the old
// neighbour was (and no other slot can tie below j).  Otherwise the old value stays as a LOWER BOUND of the row's
// nearest distance and the row is marked stale: it is scanned again only if it comes up as the lowest entry.
AG_HD void ag_repair(double nd, int i, int j, double* nn_val, int* nn_idx, int* stale) {
    const int cur = *nn_idx;
    const double val = *nn_val;
    if (cur == i || cur == j) {
        if (nd < val || (nd == val && cur == j)) {
            *nn_val = nd;
            *nn_idx = j;
        } else {
            *nn_idx = j;
            *stale = 1;
        }
    } else if (ag_better(nd, j, val, cur < 0 ? AG_NONE : cur)) {
        *nn_val = nd;
        *nn_idx = j;
    }
}
