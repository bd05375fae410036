// Centroid-linkage agglomerative clustering of unit rows, float64: the ONE text of its arithmetic and decisions.
// k_agglo.hip (the kernels behind dz_agglo_linkage) and agglo.cpp (dz_agglo_linkage_host, backend="core") compile it,
// so the host and the device round alike and cannot disagree at a tie: the leaf functions, then the merge loop itself
// (ag_scan, ag_merge_steps), which both sides run through a team of lanes.  DESIGN.md 4.24.
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

// rows_off (n_files + 1): file f owns rows rows_off[f] .. rows_off[f + 1] - 1 -- an ascending list from 0
AG_HD bool ag_offsets_ok(int n_files, const int* rows_off) {
    bool ok = rows_off[0] == 0;
    for (int f = 0; f < n_files; ++f) ok = ok && rows_off[f + 1] >= rows_off[f];
    return ok;
}

// The merge loop, run by a TEAM of lanes on the state of one file (above) and its Z:
struct AgSlots {
    double* nn_val;
    int *nn_idx, *size, *id, *active, *stale;
    double *mat, *z;
};
// A team is a policy: lane() of lanes() (lane l takes elements l, l + lanes(), ... of a list; lane 0 writes what one
// lane writes), barrier(), and lowest(v, idx): the lowest (value, index) of the lanes' pairs, in every lane (it may hold
// barriers: all lanes call it).  The device's team is a workgroup (k_agglo.hip), the host's is AgOneLane.  They decide
// alike because `lowest` is a lexicographic minimum -- lower value, then lower index, NaN never wins (ag_take) -- which
// is exact, associative and commutative: however the list is dealt to the lanes, the result is the pair one lane finds
// walking it alone.  Everything else is per element k, from values no lane writes in the same phase.  This is the only
// reason one text can serve both.
struct AgOneLane {
    AG_HD int lane() const { return 0; }
    AG_HD int lanes() const { return 1; }
    AG_HD void barrier() const {}
    AG_HD void lowest(double&, int&) const {}
};

// Row k scanned by the team: its nearest active slot above it, written by lane 0, and the row is exact again.  Call
// from all lanes; the entry is visible to them after the next barrier.
template <typename Team>
AG_HD void ag_scan(const AgSlots& s, int k, int n, Team team) {
    const double* row = s.mat + (long long)k * n;
    double best = INFINITY;
    int bidx = AG_NONE;
    for (int m = k + 1 + team.lane(); m < n; m += team.lanes())
        if (s.active[m]) ag_take(row[m], m, best, bidx);
    team.lowest(best, bidx);
    if (team.lane() == 0) {
        s.nn_val[k] = best;
        s.nn_idx[k] = bidx == AG_NONE ? -1 : bidx;
        s.stale[k] = 0;
    }
}

// Merges t, t + 1, ... of a file of n >= 2 slots: at most nsteps of them, up to the last one (n - 2).  Returns the next
// merge.  *bad: an index failed its range check at the merge returned, and the file ends there.
// Every value a branch below depends on is the same in all lanes of the team (read after a barrier from memory that no
// lane writes before the next one), so every barrier is reached by all of them.
template <typename Team>
AG_HD int ag_merge_steps(const AgSlots& s, int n, int t, int nsteps, bool* bad_out, Team team) {
    const int lane = team.lane(), nl = team.lanes();
    bool bad = false;
    for (int it = 0; it < nsteps && t < n - 1; ++it, ++t) {
        // the lowest (nn_val, i) whose row is exact
        double dij;
        int i;
        for (int tries = 0;; ++tries) {
            dij = INFINITY;
            i = AG_NONE;
            for (int k = lane; k < n; k += nl) ag_take(s.nn_val[k], k, dij, i);
            team.lowest(dij, i);
            bad = i < 0 || i >= n || tries > n;
            if (bad || !s.stale[i]) break;
            ag_scan(s, i, n, team);
            team.barrier();
        }
        const int j = bad ? -1 : s.nn_idx[i];
        bad = bad || !ag_pair_ok(i, j, dij, n, s.active);
        if (bad) break;
        const int ni = s.size[i], nj = s.size[j], id_i = s.id[i], id_j = s.id[j];
        team.barrier();                           // everyone has read slot i and j's state
        if (lane == 0) {
            ag_z_row(s.z + (long long)t * 4, id_i, id_j, dij, ni + nj);
            s.size[j] = ni + nj;
            s.id[j] = n + t;
            s.active[i] = 0;
            s.nn_val[i] = INFINITY;
            s.nn_idx[i] = -1;
            s.stale[i] = 0;
        }
        team.barrier();
        // Lance-Williams on row and column j, and the entries of the rows below j
        const double* row_i = s.mat + (long long)i * n;
        double* row_j = s.mat + (long long)j * n;
        for (int k = lane; k < n; k += nl) {
            if (k == i || k == j || !s.active[k]) continue;
            const double nd = ag_lance_williams(row_i[k], row_j[k], dij, ni, nj);
            row_j[k] = nd;
            s.mat[(long long)k * n + j] = nd;
            if (k < j) ag_repair(nd, i, j, &s.nn_val[k], &s.nn_idx[k], &s.stale[k]);
        }
        team.barrier();
        ag_scan(s, j, n, team);
        team.barrier();
    }
    *bad_out = bad;
    return t;
}
