// Whole-file diarization, the host half: everything after the dendrogram -- the cut, the ranking of
// the flat clusters, their centroids, the assignment of every usable row and the reconstruction of the timeline -- and
// the linkage itself from the text of agglo_core.h, which is what backend="core" and a machine without a GPU run.
//   dz_agglo_linkage_host   Z of every file, files on the host pool
//   dz_agglo_cut            scipy's fcluster(Z, threshold, "distance"), then the kept clusters
//   dz_offline_assign       rows -> nearest kept centroid (cosine)
//   dz_offline_reconstruct  (chunks, frames, local speakers) scores + assignments -> (frames, clusters) activity
#include "agglo_core.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/diart_amd.h"
#include "hostpool.h"

void dz_set_error(const char* fmt, ...);

namespace {

// One file's linkage: x (n, D) -> Z (n - 1, 4).  The distance matrix is built here; the slots, the selection and the
// repairs are agglo_core.h's merge loop, the text agglo_merge_kernel runs, on a team of one lane.
int linkage_one(const double* x, int n, int D, double* Z) {
    if (n < 2) return AG_OK;
    std::vector<double> mat((size_t)n * n), nn_val(n);
    std::vector<int> nn_idx(n), size(n, 1), id(n), active(n, 1), stale(n, 0);
    // the upper half four columns at a time (four independent chains, each adding its terms in ascending k), mirrored:
    // (a - b)^2 and (b - a)^2 are the same double
    for (int r = 0; r < n; ++r) {
        const double* a = x + (size_t)r * D;
        mat[(size_t)r * n + r] = 0.0;
        int c = r + 1;
        for (; c + 3 < n; c += 4) {
            const double *b0 = x + (size_t)c * D, *b1 = b0 + D, *b2 = b1 + D, *b3 = b2 + D;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int k = 0; k < D; ++k) {
                s0 = ag_d2_term(s0, a[k], b0[k]);
                s1 = ag_d2_term(s1, a[k], b1[k]);
                s2 = ag_d2_term(s2, a[k], b2[k]);
                s3 = ag_d2_term(s3, a[k], b3[k]);
            }
            const double s[4] = {s0, s1, s2, s3};
            for (int u = 0; u < 4; ++u) mat[(size_t)r * n + c + u] = mat[(size_t)(c + u) * n + r] = s[u];
        }
        for (; c < n; ++c) {
            double s = 0.0;
            for (int k = 0; k < D; ++k) s = ag_d2_term(s, a[k], x[(size_t)c * D + k]);
            mat[(size_t)r * n + c] = mat[(size_t)c * n + r] = s;
        }
    }
    const AgSlots s = {nn_val.data(), nn_idx.data(), size.data(), id.data(), active.data(), stale.data(), mat.data(), Z};
    for (int k = 0; k < n; ++k) {
        id[k] = k;
        ag_scan(s, k, n, AgOneLane{});
    }
    bool bad = false;
    const int t = ag_merge_steps(s, n, 0, n - 1, &bad, AgOneLane{});
    return bad ? t : AG_OK;
}

}  // namespace

extern "C" int dz_agglo_linkage_host(int n_files, const int* rows_off, const double* x, int D, double* Z, int* status,
                                     int num_threads) {
    if (!rows_off || !status || n_files < 1) {
        dz_set_error("dz_agglo_linkage_host: NULL argument or no file");
        return 2;
    }
    if (D < 1 || D > AG_DMAX) {
        dz_set_error("dz_agglo_linkage_host: dimension %d outside [1, %d]", D, AG_DMAX);
        return 2;
    }
    if (!ag_offsets_ok(n_files, rows_off)) {
        dz_set_error("dz_agglo_linkage_host: rows_off is no ascending list from 0");
        return 2;
    }
    std::vector<long long> z_off(n_files + 1, 0);
    for (int f = 0; f < n_files; ++f) {
        const int n = rows_off[f + 1] - rows_off[f];
        z_off[f + 1] = z_off[f] + (n > 1 ? n - 1 : 0);
    }
    if (z_off[n_files] > 0 && (!x || !Z)) {
        dz_set_error("dz_agglo_linkage_host: NULL argument");
        return 2;
    }
    const dz_host_failure fail = dz_host_parallel_rc(n_files, dz_host_threads(num_threads, n_files), [&](int, int f) {
        const int n = rows_off[f + 1] - rows_off[f];
        try {
            status[f] = linkage_one(x + (size_t)rows_off[f] * D, n, D, Z + z_off[f] * 4);
        } catch (const std::bad_alloc&) {
            dz_set_error("dz_agglo_linkage_host: no memory for the %d x %d matrix of file %d", n, n, f);
            return 1;
        }
        return 0;
    });
    if (fail.code != 0) {
        dz_set_error("%s", fail.message.c_str());
        return fail.code;
    }
    return 0;
}

// labels (n): the kept cluster 0 .. G - 1 of each leaf, or -1 (its flat cluster was not kept); *n_kept = G.
static int cut_impl(const double* Z, int n, double threshold, int min_cluster_size, int max_speakers, int* labels, int* n_kept) {
    if (!n_kept || n < 0 || (n > 0 && !labels) || (n > 1 && !Z)) {
        dz_set_error("dz_agglo_cut: NULL argument or %d leaves", n);
        return 2;
    }
    if (!std::isfinite(threshold) || min_cluster_size < 1 || max_speakers < 1) {
        dz_set_error("dz_agglo_cut: threshold %g must be finite, min_cluster_size %d and max_speakers %d at least 1", threshold,
                     min_cluster_size, max_speakers);
        return 2;
    }
    *n_kept = 0;
    if (n == 0) return 0;
    // a valid dendrogram: merge t joins two nodes below n + t, each node is joined once
    const int nodes = 2 * n - 1;
    std::vector<int> left(n > 1 ? n - 1 : 0), right(n > 1 ? n - 1 : 0);
    std::vector<char> used(nodes, 0);
    std::vector<double> top(nodes, 0.0);        // the highest merge of the node's subtree (leaves: none)
    for (int t = 0; t < n - 1; ++t) {
        const double a = Z[(size_t)t * 4], b = Z[(size_t)t * 4 + 1], h = Z[(size_t)t * 4 + 2];
        if (!(a >= 0 && a < n + t && b >= 0 && b < n + t) || a != std::floor(a) || b != std::floor(b) || a == b || !(h >= 0) ||
            used[(int)a] || used[(int)b]) {
            dz_set_error("dz_agglo_cut: row %d of Z (%g, %g, %g) is no merge of a dendrogram over %d leaves", t, a, b, h, n);
            return 2;
        }
        left[t] = (int)a;
        right[t] = (int)b;
        used[left[t]] = used[right[t]] = 1;
        top[n + t] = std::max(h, std::max(top[left[t]], top[right[t]]));
    }
    // flat clusters: the maximal subtrees whose merges are all at or below the threshold
    std::vector<int> flat(n, -1), stack;
    int n_flat = 0;
    std::vector<std::pair<int, int>> walk;      // (node, flat cluster or -1)
    walk.emplace_back(nodes - 1, -1);
    while (!walk.empty()) {
        const auto [node, in] = walk.back();
        walk.pop_back();
        int c = in;
        if (c < 0 && (node < n || top[node] <= threshold)) c = n_flat++;
        if (node < n) {
            flat[node] = c;
        } else {
            walk.emplace_back(left[node - n], c);
            walk.emplace_back(right[node - n], c);
        }
    }
    std::vector<int> count(n_flat, 0), first(n_flat, n);
    for (int r = 0; r < n; ++r) {
        ++count[flat[r]];
        first[flat[r]] = std::min(first[flat[r]], r);
    }
    std::vector<int> rank(n_flat);
    for (int c = 0; c < n_flat; ++c) rank[c] = c;
    std::sort(rank.begin(), rank.end(), [&](int a, int b) { return count[a] != count[b] ? count[a] > count[b] : first[a] < first[b]; });
    std::vector<int> kept;
    for (int c : rank)
        if (count[c] >= min_cluster_size && (int)kept.size() < max_speakers) kept.push_back(c);
    if (kept.empty()) kept.push_back(rank[0]);
    std::sort(kept.begin(), kept.end(), [&](int a, int b) { return first[a] < first[b]; });
    std::vector<int> number(n_flat, -1);
    for (size_t g = 0; g < kept.size(); ++g) number[kept[g]] = (int)g;
    for (int r = 0; r < n; ++r) labels[r] = number[flat[r]];
    *n_kept = (int)kept.size();
    return 0;
}

// x (rows, D) unit rows; train (n_train) their indices that were clustered, labels (n_train) from dz_agglo_cut.  Cluster
// g's centroid is the mean of its own train members (added in their order); a row goes to the centroid at the lowest
// cosine distance 1 - x.c / |c| (ties: the lowest g).  assign (rows).
static int assign_impl(const double* x, int rows, int D, const int* train, const int* labels, int n_train, int n_kept,
                       int* assign, double* centroids) {
    if (rows < 0 || n_train < 0 || n_kept < 0 || D < 1 || (rows > 0 && (!x || !assign)) || (n_train > 0 && (!train || !labels)) ||
        (n_kept > 0 && !centroids)) {
        dz_set_error("dz_offline_assign: NULL argument or a negative count");
        return 2;
    }
    std::vector<int> members(n_kept, 0);
    for (size_t e = 0; e < (size_t)n_kept * D; ++e) centroids[e] = 0.0;
    for (int m = 0; m < n_train; ++m) {
        const int g = labels[m], r = train[m];
        if (g >= n_kept || r < 0 || r >= rows) {
            dz_set_error("dz_offline_assign: train row %d (row %d, cluster %d) outside %d rows / %d clusters", m, r, g, rows, n_kept);
            return 2;
        }
        if (g < 0) continue;
        ++members[g];
        for (int k = 0; k < D; ++k) centroids[(size_t)g * D + k] += x[(size_t)r * D + k];
    }
    std::vector<double> norm(n_kept);
    for (int g = 0; g < n_kept; ++g) {
        if (members[g] == 0) {
            dz_set_error("dz_offline_assign: cluster %d has no train row", g);
            return 2;
        }
        double s = 0.0;
        for (int k = 0; k < D; ++k) {
            centroids[(size_t)g * D + k] /= (double)members[g];
            s += centroids[(size_t)g * D + k] * centroids[(size_t)g * D + k];
        }
        norm[g] = std::sqrt(s);
    }
    for (int r = 0; r < rows; ++r) {
        double best = INFINITY;
        int bg = AG_NONE;
        for (int g = 0; g < n_kept; ++g) {
            double dot = 0.0;
            for (int k = 0; k < D; ++k) dot += x[(size_t)r * D + k] * centroids[(size_t)g * D + k];
            const double d = 1.0 - dot / norm[g];
            if (bg == AG_NONE || d < best) {           // a NaN distance (a zero centroid) never wins over a number
                if (d == d || bg == AG_NONE) {
                    best = d;
                    bg = g;
                }
            }
        }
        assign[r] = bg == AG_NONE ? -1 : bg;
    }
    return 0;
}

// The entry points keep std::bad_alloc on this side of the C boundary, as dz_agglo_linkage_host does.
extern "C" int dz_agglo_cut(const double* Z, int n, double threshold, int min_cluster_size, int max_speakers, int* labels,
                            int* n_kept) {
    try {
        return cut_impl(Z, n, threshold, min_cluster_size, max_speakers, labels, n_kept);
    } catch (const std::bad_alloc&) {
        dz_set_error("dz_agglo_cut: no memory for a dendrogram over %d leaves", n);
        return 1;
    }
}

extern "C" int dz_offline_assign(const double* x, int rows, int D, const int* train, const int* labels, int n_train,
                                 int n_kept, int* assign, double* centroids) {
    try {
        return assign_impl(x, rows, D, train, labels, n_train, n_kept, assign, centroids);
    } catch (const std::bad_alloc&) {
        dz_set_error("dz_offline_assign: no memory for %d clusters", n_kept);
        return 1;
    }
}

// Per file: seg (C, F, K) scores, assign (C, K) cluster of each local speaker or -1, offset (C) first output frame of
// each chunk, G clusters, T output frames -> active (T, G) bytes.
extern "C" int dz_offline_reconstruct(int n_files, const float* const* seg, const int* const* assign, const int* const* offset,
                                      const int* chunks, int F, int K, const int* n_kept, double tau_active, const int* frames,
                                      unsigned char* const* active, int num_threads) {
    if (n_files < 1 || !seg || !assign || !offset || !chunks || !n_kept || !frames || !active || F < 1 || K < 1) {
        dz_set_error("dz_offline_reconstruct: NULL argument, no file, or %d frames x %d local speakers", F, K);
        return 2;
    }
    for (int f = 0; f < n_files; ++f) {
        if (chunks[f] < 0 || n_kept[f] < 0 || frames[f] < 0 || (chunks[f] > 0 && (!seg[f] || !assign[f] || !offset[f])) ||
            ((long long)frames[f] * n_kept[f] > 0 && !active[f])) {
            dz_set_error("dz_offline_reconstruct: file %d: NULL argument or a negative count", f);
            return 2;
        }
        for (int c = 0; c < chunks[f]; ++c) {
            if (offset[f][c] < 0 || (long long)offset[f][c] + F > frames[f]) {
                dz_set_error("dz_offline_reconstruct: file %d: chunk %d at frame %d leaves the %d output frames", f, c,
                             offset[f][c], frames[f]);
                return 2;
            }
            for (int k = 0; k < K; ++k)
                if (assign[f][(size_t)c * K + k] >= n_kept[f]) {
                    dz_set_error("dz_offline_reconstruct: file %d: chunk %d speaker %d in cluster %d of %d", f, c, k,
                                 assign[f][(size_t)c * K + k], n_kept[f]);
                    return 2;
                }
        }
    }
    const auto one_file = [&](int f) {
        const int C = chunks[f], G = n_kept[f], T = frames[f];
        if ((long long)T * G == 0) return;
        std::vector<double> A((size_t)T * G, 0.0), on_sum(T, 0.0), a(G);
        std::vector<int> cover(T, 0), order(G);
        for (int c = 0; c < C; ++c) {
            const float* s = seg[f] + (size_t)c * F * K;
            bool valid = true;
            for (size_t e = 0; e < (size_t)F * K && valid; ++e) valid = std::isfinite(s[e]);
            if (!valid) continue;
            const int* as = assign[f] + (size_t)c * K;
            for (int fr = 0; fr < F; ++fr) {
                const int t = offset[f][c] + fr;
                std::fill(a.begin(), a.end(), -INFINITY);     // no local speaker of the cluster yet
                int on = 0;
                for (int k = 0; k < K; ++k) {
                    const double v = (double)s[(size_t)fr * K + k];
                    on += v > tau_active;
                    if (as[k] >= 0 && v > a[as[k]]) a[as[k]] = v;
                }
                for (int g = 0; g < G; ++g) A[(size_t)t * G + g] += a[g] == -INFINITY ? 0.0 : a[g];
                on_sum[t] += (double)on;
                ++cover[t];
            }
        }
        for (int t = 0; t < T; ++t) {
            unsigned char* out = active[f] + (size_t)t * G;
            std::fill(out, out + G, (unsigned char)0);
            if (cover[t] == 0) continue;
            const double mean = std::nearbyint(on_sum[t] / (double)cover[t]);     // half to even
            const int count = mean < (double)G ? (int)mean : G;
            const double* row = A.data() + (size_t)t * G;
            for (int g = 0; g < G; ++g) order[g] = g;
            std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return row[p] > row[q]; });
            for (int r = 0; r < count; ++r)
                if (row[order[r]] > 0.0) out[order[r]] = 1;
        }
    };
    const dz_host_failure fail = dz_host_parallel_rc(n_files, dz_host_threads(num_threads, n_files), [&](int, int f) {
        try {
            one_file(f);
        } catch (const std::bad_alloc&) {
            dz_set_error("dz_offline_reconstruct: no memory for the %d x %d frames of file %d", frames[f], n_kept[f], f);
            return 1;
        }
        return 0;
    });
    if (fail.code != 0) {
        dz_set_error("%s", fail.message.c_str());
        return fail.code;
    }
    return 0;
}
