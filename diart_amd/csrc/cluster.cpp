// Host side of the incremental speaker clustering, fp64 like the reference: the dz_clu handle around the decision
// core of clu_core.h (the LSAP, the SpeakerMap algebra, identify's decisions; the tuner's GPU kernel compiles the same
// text).  What is here is what a handle adds to it: the heap-backed store, so that no K, G or nr x nc is too large;
// the float32 statistics identify takes from `seg` (/root/reference/src/diart/blocks/clustering.py:137-145); the
// K x G cosine distance map (:161-166); the centroids, which take the decided updates and additions (:85-117); the
// scores (/root/reference/src/diart/mapping.py:341-360 apply); the batch over N handles on the host pool.
#include "../../include/diart_amd.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "clu_core.h"
#include "hostpool.h"

#pragma clang fp contract(off)

void dz_set_error(const char* fmt, ...);

namespace {

// The host store of the core: every array on the heap, sized by size_step / size_work from the K and G at hand.
template <typename T>
struct HeapArr {
    T* p = nullptr;
    HeapArr() = default;
    HeapArr(const HeapArr&) = delete;
    HeapArr& operator=(const HeapArr&) = delete;
    ~HeapArr() { delete[] p; }
    void size(size_t n) {
        delete[] p;
        p = nullptr;
        p = new T[n];
    }
    TC_HD operator T*() const { return p; }
};
struct CluFlags {
    HeapArr<char> on;   // on[g]: centroid g is in use
    TC_HD bool test(int g) const { return on[g]; }
    TC_HD void set(int g) { on[g] = 1; }
    TC_HD void clear(int G) {
        for (int g = 0; g < G; ++g) on[g] = 0;
    }
    TC_HD int first_free(int G) const {   // clustering.py:68-71
        for (int c = 0; c < G; ++c)
            if (!on[c]) return c;
        return -1;
    }
};
struct CluHeap {
    template <typename T> using PerK = HeapArr<T>;
    template <typename T> using PerG = HeapArr<T>;
    template <typename T> using PerKG = HeapArr<T>;
    using Active = CluFlags;
    using Index = size_t;
    static constexpr int err(int cause) { return cause; }
};

void size_work(TcLsapWork<CluHeap>& w, int K, int G) {
    const size_t M = (size_t)std::max(K, G);
    w.u.size(M); w.v.size(M); w.spc.size(M); w.temp.size((size_t)K * G);
    w.path.size(M); w.col4row.size(M); w.row4col.size(M); w.remaining.size(M);
    w.pr.size(M); w.pc.size(M); w.SR.size(M); w.SC.size(M);
}
void size_step(TcStep<CluHeap>& s, int K, int G) {   // `active` is the handle's state: sized when it is created
    const size_t M = (size_t)std::max(K, G);
    for (TcMap<CluHeap>* m : {&s.dist, &s.valid}) {
        m->m.size((size_t)K * G);
        m->raw.size(M);
    }
    size_work(s.work, K, G);
    s.un.size(K); s.cn.size(G);
    s.is_active.size(K); s.is_long.size(K); s.upd.size(K); s.add.size(K); s.assign.size(K);
    s.src.size(M); s.tgt.size(M); s.pref.size(M);
    s.missed.size(K); s.is_missed.size(K); s.newc.size(K);
}

}  // namespace

struct dz_clu {
    double tau, rho, delta;
    int G;
    int D = 0;
    int K = 0;   // the local speakers `s` is sized for
    bool has_centers = false;
    std::vector<double> centers;  // G x D
    TcStep<CluHeap> s;            // the active set (s.active), and the step's scratch: a step allocates nothing
    // blocked_centers is never populated by the reference (clustering.py:46,83)
};

namespace {

// clustering.py:119-218 + mapping.py apply.  Returns 0 ok; 3 = the reference would raise (assert / scipy error).
int step(dz_clu* c, const float* seg, int F, int K, const float* emb, int D, double* scores, int* assign) {
    if (c->has_centers && D != c->D) {
        dz_set_error("clustering: embedding dimension changed from %d to %d", c->D, D);
        return 2;
    }
    const int G = c->G;
    TcStep<CluHeap>& s = c->s;
    if (K != c->K) {
        c->K = 0;   // (not sized for any K while the arrays are replaced)
        size_step(s, K, G);
        c->K = K;
    }

    // :137-145  active: max_f >= tau ; long: mean_f >= rho (float32 arithmetic, like numpy
    // on the float32 segmentation array) ; drop speakers with NaN embeddings
    const float tau32 = (float)c->tau, rho32 = (float)c->rho;
    for (int k = 0; k < K; ++k) {
        float mx = seg[k], sum = 0.f;
        bool nanmax = false;
        for (int f = 0; f < F; ++f) {
            const float x = seg[(size_t)f * K + k];
            if (x != x) nanmax = true;
            if (x > mx) mx = x;
            sum += x;
        }
        const float mean = sum / (float)F;
        const bool act = !nanmax && (mx >= tau32);
        s.is_long[k] = (mean >= rho32) ? 1 : 0;
        bool has_nan = false;
        for (int d = 0; d < D; ++d) {
            const float e = emb[(size_t)k * D + d];
            if (e != e) { has_nan = true; break; }
        }
        s.is_active[k] = (act && !has_nan) ? 1 : 0;
    }

    int rc;
    if (!c->has_centers) {  // :149-158
        c->D = D;
        c->centers.assign((size_t)G * D, 0.0);
        c->has_centers = true;
        rc = tc_decide_first(s, K, G);
    } else {
        // :161-166  cosine distance map; only the pairs of an active speaker and an active centroid are computed,
        // the others are the sentinel the reference overwrites them with
        for (int g = 0; g < G; ++g)
            if (s.active.test(g)) s.cn[g] = tc_sqrt(tc_dot2_vv(&c->centers[(size_t)g * D], 1, D));
        for (int k = 0; k < K; ++k)
            if (s.is_active[k]) s.un[k] = tc_sqrt(tc_dot2_ff(emb + (size_t)k * D, D));
        tc_map_init(s.dist, K, G);
        for (int k = 0; k < K; ++k)
            for (int g = 0; g < G && s.is_active[k]; ++g)
                if (s.active.test(g))
                    s.dist.m[(size_t)k * G + g] =
                        tc_cosine(tc_dot2_fv(emb + (size_t)k * D, &c->centers[(size_t)g * D], 1, D), s.un[k], s.cn[g]);
        rc = tc_decide(s, K, G, c->delta);
    }
    // :197-208  On an error too: the reference updates pair by pair and raises mid-loop, and upd / add hold what was
    // decided up to there.
    for (int k = 0; k < K; ++k) {
        const int gu = s.upd[k], ga = s.add[k];
        const float* e = emb + (size_t)k * D;
        if (gu >= 0)
            for (int d = 0; d < D; ++d) c->centers[(size_t)gu * D + d] += (double)e[d];
        if (ga >= 0)
            for (int d = 0; d < D; ++d) c->centers[(size_t)ga * D + d] = (double)e[d];
    }
    if (rc) {
        dz_set_error(rc == TC_ERR_UNKNOWN ? "Cannot update unknown centers"
                     : rc == TC_ERR_FULL  ? "clustering: no free center"
                                          : "clustering: cost matrix contains invalid numeric entries");
        return 3;
    }
    // mapping.py:341-360 apply
    if (assign)
        for (int k = 0; k < K; ++k) assign[k] = s.assign[k];
    if (scores) {
        std::memset(scores, 0, sizeof(double) * (size_t)F * G);
        for (int k = 0; k < K; ++k) {
            const int t = s.assign[k];
            if (t < 0) continue;
            for (int f = 0; f < F; ++f) scores[(size_t)f * G + t] = (double)seg[(size_t)f * K + k];
        }
    }
    return 0;
}

}  // namespace

extern "C" int dz_clu_create(double tau_active, double rho_update, double delta_new,
                             int max_speakers, dz_clu** out) {
    if (!out || max_speakers < 1) {
        dz_set_error("dz_clu_create: bad arguments");
        return 2;
    }
    dz_clu* c = new (std::nothrow) dz_clu;
    if (!c) {
        dz_set_error("dz_clu_create: out of memory");
        return 1;
    }
    c->tau = tau_active; c->rho = rho_update; c->delta = delta_new; c->G = max_speakers;
    c->s.active.on.size(max_speakers);
    c->s.active.clear(max_speakers);
    *out = c;
    return 0;
}
extern "C" int dz_clu_reset(dz_clu* c) {
    if (!c) return 2;
    c->has_centers = false;
    c->D = 0;
    c->centers.clear();
    c->s.active.clear(c->G);
    return 0;
}
extern "C" int dz_clu_destroy(dz_clu* c) {
    delete c;
    return 0;
}
extern "C" int dz_clu_step(dz_clu* c, const float* seg, int frames, int k_local, const float* emb,
                           int dim, double* scores_out, int* assign_out) {
    if (!c || !seg || !emb || frames < 1 || k_local < 1 || dim < 1) {
        dz_set_error("dz_clu_step: bad arguments");
        return 2;
    }
    return step(c, seg, frames, k_local, emb, dim, scores_out, assign_out);
}
extern "C" int dz_clu_step_batch(dz_clu** clus, int n, const float* seg, int frames, int k_local,
                                 const float* emb, int dim, double* scores_out, int* assign_out,
                                 int num_threads) {
    if (!clus || n < 1 || !seg || !emb || frames < 1 || k_local < 1 || dim < 1) {
        dz_set_error("dz_clu_step_batch: bad arguments");
        return 2;
    }
    const int G = clus[0]->G;
    for (int i = 0; i < n; ++i)
        if (!clus[i] || clus[i]->G != G) {
            dz_set_error("dz_clu_step_batch: handles must share max_speakers");
            return 2;
        }
    // Streams are independent, so on the pool the ones that succeeded HAVE been stepped; the caller decides what to
    // do with the failed ones.  On one thread the first failure ends the call with the step's own message.
    const dz_host_failure f = dz_host_parallel_rc(n, num_threads, [&](int, int i) {
        return step(clus[i], seg + (size_t)i * frames * k_local, frames, k_local,
                    emb + (size_t)i * k_local * dim, dim,
                    scores_out ? scores_out + (size_t)i * frames * G : nullptr,
                    assign_out ? assign_out + (size_t)i * k_local : nullptr);
    });
    if (f.code && dz_host_threads(num_threads, n) > 1)
        dz_set_error("dz_clu_step_batch: stream %d of %d failed (code %d): %s%s", f.index, n, f.code, f.message.c_str(),
                     f.failed > 1 ? " (other streams failed too)" : "");
    return f.code;
}
extern "C" int dz_clu_get_centers(dz_clu* c, double* out, int dim) {
    if (!c) return 2;
    if (!c->has_centers) return 1;
    if (dim != c->D || !out) {
        dz_set_error("dz_clu_get_centers: dim %d != %d", dim, c->D);
        return 2;
    }
    std::memcpy(out, c->centers.data(), sizeof(double) * c->centers.size());
    return 0;
}
extern "C" int dz_clu_get_active(dz_clu* c, int* out_mask) {
    if (!c || !out_mask) return 2;
    for (int g = 0; g < c->G; ++g) out_mask[g] = c->s.active.test(g) ? 1 : 0;
    return 0;
}
extern "C" int dz_clu_dim(dz_clu* c) { return (c && c->has_centers) ? c->D : 0; }
extern "C" int dz_clu_set_state(dz_clu* c, const double* centers, const int* active_mask, int dim) {
    if (!c || !centers || !active_mask || dim < 1) {
        dz_set_error("dz_clu_set_state: bad arguments");
        return 2;
    }
    c->D = dim;
    c->centers.assign(centers, centers + (size_t)c->G * dim);
    for (int g = 0; g < c->G; ++g) c->s.active.on[g] = active_mask[g] ? 1 : 0;
    c->has_centers = true;
    return 0;
}
extern "C" int dz_lsap(const double* cost, int nr, int nc, int* col4row) {
    TcLsapWork<CluHeap> w;
    size_work(w, nr, nc);
    std::vector<int> raw(std::min(nr, nc));
    int nraw;
    const int rc = tc_lsap(cost, nr, nc, raw.data(), &nraw, w);
    if (rc) {
        dz_set_error(rc == 1 ? "matrix contains invalid numeric entries" : "cost matrix is infeasible");
        return rc;
    }
    // raw holds the columns of the pairs sorted by row: every row has one, or (nc < nr) their rows are w.pr
    for (int r = 0; r < nr; ++r) col4row[r] = -1;
    for (int i = 0; i < nraw; ++i) col4row[nc < nr ? w.pr[i] : i] = raw[i];
    return 0;
}
