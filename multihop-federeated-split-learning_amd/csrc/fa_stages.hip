// fa_stages.hip -- the aggregation stages of libfa (fa.h: server optimizer, clip, Krum, DnC, geomed, Bulyan, noise, MX8
// receipts, MX8 replies, secagg) and their entries of the C ABI.  A stage is one struct (fa_host.h), one row of the admission
// rule (kRules, admit), its set_part_* / free_* pair, and its share of the four calls reduce_part (fa_api.hip) makes
// around a range part's launches: stage_round_begin, stage_piece, stage_gpu_end, stage_round_end.
#include "fa_host.h"

namespace fah {

// ------------------------------------------------------------------ server optimizer

inline bool opt_adaptive(int rule) { return rule == FA_OPT_ADAGRAD || rule == FA_OPT_ADAM || rule == FA_OPT_YOGI; }
inline bool finite_f(float f) { return f - f == 0.0f; }

// The refusals of fa_set_server_opt / fa_server_opt_device, naming the field.
int check_opt(const fa_server_opt& o) {
    if (o.rule < FA_OPT_NONE || o.rule > FA_OPT_YOGI) return fail(FA_ERR_ARG, "server opt: rule %d outside 0..4", o.rule);
    if (o.rule == FA_OPT_NONE) return FA_OK;
    if (!finite_f(o.lr) || o.lr < 0.0f) return fail(FA_ERR_ARG, "server opt: lr %g must be finite and >= 0", (double)o.lr);
    if (!(o.beta1 >= 0.0f && o.beta1 < 1.0f)) return fail(FA_ERR_ARG, "server opt: beta1 %g outside [0, 1)", (double)o.beta1);
    if ((o.rule == FA_OPT_ADAM || o.rule == FA_OPT_YOGI) && !(o.beta2 >= 0.0f && o.beta2 < 1.0f))
        return fail(FA_ERR_ARG, "server opt: beta2 %g outside [0, 1)", (double)o.beta2);
    if (opt_adaptive(o.rule) && (!finite_f(o.tau) || !(o.tau > 0.0f)))
        return fail(FA_ERR_ARG, "server opt: tau %g must be finite and > 0", (double)o.tau);
    return FA_OK;
}

fa::OptHyper opt_hyper(const fa_server_opt& o) {
    // c1, c2 in fp32 on the host (volatile: one rounded fp32 subtraction each, whatever the host's float mode)
    volatile float c1 = 1.0f - o.beta1, c2 = 1.0f - o.beta2;
    return fa::OptHyper{o.lr, o.beta1, o.beta2, o.tau, c1, c2};
}

// One launch of the stage on the current device: `rule` (or fa::kOptBoot) over n elements, split (fa_split.h)
// with avg in the lead -- the vector form where the state and the output allow it too.
int opt_on(const fa::Tuning& tu, int rule, const fa_server_opt& o, const float* avg, float* x, float* m, float* v,
           size_t n, void* out, fa_dtype odt, hipStream_t s) {
    if (n == 0) return FA_OK;
    fa::Split sp = fa::split_at(avg, 4, n);
    sp.require_input(x);
    sp.require_input(m);
    if (v) sp.require_input(v);
    if (out) sp.require(out, dsize(odt));
    FA_HIP(fa::launch_server_opt(rule, opt_hyper(o), avg, x, m, v, out, odt, sp, tu, s));
    return FA_OK;
}

// One launch of the noise stage on the current device: out (dtype odt; avg itself for an in-place f32 pass) :=
// avg + stddev z over n elements that are bucket elements idx0 .., split (fa_split.h) with avg in the lead.
int noise_on(const fa::Tuning& tu, const float* avg, void* out, fa_dtype odt, float stddev, uint64_t seed, uint32_t stream,
             uint32_t round, uint64_t idx0, size_t n, hipStream_t s) {
    if (n == 0) return FA_OK;
    fa::Split sp = fa::split_at(avg, 4, n);
    sp.require(out, dsize(odt));
    FA_HIP(fa::launch_noise(avg, out, odt, stddev, seed, stream, round, idx0, sp, tu, s));
    return FA_OK;
}
constexpr uint64_t kNoiseRounds = (uint64_t)1 << 32;  // rounds 0 .. 2^32 - 1 exist

// ------------------------------------------------------------------ clip stage

// Rule 2 of fa.h "Clip stage": volatile keeps each step one rounded fp64 / fp32 operation.
float clip_scale(double sumsq, float max_norm, int* excluded) {
    volatile double nrm = std::sqrt(sumsq);
    const double N = nrm;
    const bool out = N != N || N == HUGE_VAL;
    if (excluded) *excluded = out ? 1 : 0;
    if (out) return 0.0f;
    if (N <= (double)max_norm) return 1.0f;
    volatile double q = (double)max_norm / N;
    return (float)q;
}

void free_measure_scratch(MeasureScratch& m) {
    if (m.dev) (void)hipFree(m.dev);
    if (m.host) (void)hipHostFree(m.host);
    m = MeasureScratch{};
}

// Room on the current device for a measure pass of `outs` results and `parts` partials.  Never shrinks: a
// reallocation keeps the larger of the old and the new count of each.  stage: "clip: norm-pass", "krum:
// distance-pass".
int ensure_measure_scratch(MeasureScratch& m, size_t outs, size_t parts, const char* stage) {
    if (m.dev && m.outs >= outs && m.parts >= parts) return FA_OK;
    const size_t ocap = std::max<size_t>(std::max(outs, m.outs), 256), pcap = std::max<size_t>(std::max(parts, m.parts), 1);
    free_measure_scratch(m);
    const size_t dev_bytes = (ocap + pcap) * sizeof(double);
    if (hipMalloc((void**)&m.dev, dev_bytes) != hipSuccess ||
        hipHostMalloc((void**)&m.host, ocap * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (m.dev) (void)hipFree(m.dev);
        m = MeasureScratch{};
        return fail(FA_ERR_NOMEM, "%s scratch of %zu B failed", stage, dev_bytes);
    }
    m.outs = ocap;
    m.parts = pcap;
    return FA_OK;
}
constexpr size_t kClipParts = (size_t)fa::kMaxClients * (size_t)fa::kClipMaxPartials;  // the norm pass's partials
inline size_t krum_parts(int D) { return (size_t)fa::krum_pairs(D) * (size_t)fa::kKrumMaxPartials; }

// Enqueues the norm pass on the current device: d_sums[k] = Q_k of clients[k] (n elements of `in`) against ref,
// k < D, in passes of kMaxClients clients; d_part: kMaxClients * kClipMaxPartials doubles of scratch.  The
// vector form where every client and ref allow it (fa_split.h).
int clip_sumsq_on(const fa::Tuning& tu, const void* const* clients, int D, size_t n, fa_dtype in, const float* ref,
                  double* d_part, double* d_sums, hipStream_t s) {
    fa::Split sp = fa::split_at(clients[0], dsize(in), n);
    for (int k = 0; k < D; ++k) sp.require_input(clients[k]);
    sp.require(ref, 4);
    for (int k0 = 0; k0 < D; k0 += fa::kMaxClients) {
        const int nc = std::min(fa::kMaxClients, D - k0);
        const fa::ClientTable t = client_table(clients, nullptr, k0, nc);
        FA_HIP(fa::launch_clip_sumsq(t, nc, in, ref, sp, d_part, d_sums + k0, tu, s));
    }
    return FA_OK;
}

// ------------------------------------------------------------------ Krum stage

// The refusals of f and m for D clients (fa.h "Krum stage"), naming the cause; *m_out = m with -1 resolved.
int check_krum(int D, int f, int m, int* m_out) {
    if (D > FA_KRUM_MAX_CLIENTS) return fail(FA_ERR_ARG, "krum: D = %d clients (at most %d)", D, FA_KRUM_MAX_CLIENTS);
    if (f < 0 || 2 * f + 2 >= D)
        return fail(FA_ERR_ARG, "krum: f = %d does not fit D = %d clients (0 <= f and 2 f + 2 < D)", f, D);
    const int mm = m == -1 ? D - f : m;
    if (mm < 1 || mm > D - f)
        return fail(FA_ERR_ARG, "krum: m = %d does not fit D = %d, f = %d (1 <= m <= D - f, or -1 for D - f)", m, D, f);
    if (m_out) *m_out = mm;
    return FA_OK;
}

// Rules 2-3 of fa.h "Krum stage" (D, f, m checked): volatile keeps each step one rounded fp64 add.
void krum_select(const double* dist, int D, int f, int m, double* scores, int* selected, int* n_selected) {
    const double inf = HUGE_VAL;
    std::vector<double> row((size_t)D - 1), sc((size_t)D);
    for (int k = 0; k < D; ++k) {
        size_t c = 0;
        for (int j = 0; j < D; ++j) {
            if (j == k) continue;
            const double q = dist[(size_t)k * D + j];
            row[c++] = q != q ? inf : q;
        }
        std::sort(row.begin(), row.end());
        volatile double acc = 0.0;
        for (int i = 0; i < D - f - 2; ++i) acc = acc + row[(size_t)i];
        sc[(size_t)k] = acc;
    }
    std::vector<int> order((size_t)D);
    for (int k = 0; k < D; ++k) order[(size_t)k] = k;
    // by (S_k, k) ascending; a NaN score (only from a matrix holding -inf) sorts as +inf
    auto key = [&](int k) { return sc[(size_t)k] != sc[(size_t)k] ? inf : sc[(size_t)k]; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
    int ns = 0;
    for (int k = 0; k < D; ++k) {
        if (scores) scores[k] = sc[(size_t)k];
        if (selected) selected[k] = 0;
    }
    for (int i = 0; i < m; ++i) {
        const int k = order[(size_t)i];
        if (!(sc[(size_t)k] < inf)) break;  // +inf is never selected, nor anything after it
        if (selected) selected[k] = 1;
        ++ns;
    }
    if (n_selected) *n_selected = ns;
}

// Rule 4: the weights of a round whose selection is `selected` (w_out[k] is set for every k; only the selected
// ones enter the chain).
void krum_weights(const float* w, const int* selected, int D, float* w_out) {
    volatile double W = 0.0, Ws = 0.0;
    int ns = 0;
    for (int k = 0; k < D; ++k) {
        W = W + (double)w[k];
        if (selected[k]) {
            Ws = Ws + (double)w[k];
            ++ns;
        }
    }
    volatile double ratio = 0.0;
    bool plain = ns == D || !(Ws > 0.0);
    if (!plain) {
        ratio = W / Ws;
        const double r = ratio;
        plain = r != r || r == HUGE_VAL || r == -HUGE_VAL;
    }
    for (int k = 0; k < D; ++k) {
        if (plain) {
            w_out[k] = w[k];
        } else {
            volatile double prod = (double)w[k] * ratio;
            w_out[k] = (float)prod;
        }
    }
}

// Enqueues the distance pass on the current device: d_dist (D * D doubles) = the matrix of clients[0..D) (n > 0
// elements of `in`); d_part: the partials scratch.  The vector form where every client allows it (fa_split.h).
int pairdist_on(const fa::Tuning& tu, const void* const* clients, int D, size_t n, fa_dtype in, double* d_part,
                double* d_dist, hipStream_t s) {
    fa::Split sp = fa::split_at(clients[0], dsize(in), n);
    for (int k = 0; k < D; ++k) sp.require_input(clients[k]);
    const fa::ClientTable t = client_table(clients, nullptr, 0, D);
    FA_HIP(fa::launch_pairdist(t, D, in, sp, d_part, d_dist, tu, s));
    return FA_OK;
}

// ------------------------------------------------------------------ DnC stage

inline size_t gram_parts(int D) { return (size_t)fa::gram_entries(D) * (size_t)fa::kGramMaxPartials; }

// The refusals of drop and P for D clients (fa.h "DnC stage"), naming the cause.
int check_dnc(int D, int drop, int iters) {
    if (D > FA_DNC_MAX_CLIENTS) return fail(FA_ERR_ARG, "dnc: D = %d clients (at most %d)", D, FA_DNC_MAX_CLIENTS);
    if (drop < 0 || 2 * drop >= D)
        return fail(FA_ERR_ARG, "dnc: drop = %d does not fit D = %d clients (0 <= drop and 2 drop < D)", drop, D);
    if (iters < 1 || iters > FA_DNC_MAX_ITERS) return fail(FA_ERR_ARG, "dnc: iters = %d outside 1..%d", iters, FA_DNC_MAX_ITERS);
    return FA_OK;
}

// One rounded fp64 operation each, whatever the host's contraction mode.
inline double add_r(double a, double b) {
    volatile double r = a + b;
    return r;
}
inline double mul_r(double a, double b) {
    volatile double r = a * b;
    return r;
}
inline double div_r(double a, double b) {
    volatile double r = a / b;
    return r;
}

// Rules 2-7 of fa.h "DnC stage" (D, drop, iters checked): scores and selected hold D entries each, any may be null.
void dnc_select(const double* gram, int D, int drop, int iters, double* scores, int* selected, int* n_selected) {
    const double inf = HUGE_VAL;
    const size_t n = (size_t)D;
    std::vector<int> R;
    for (int k = 0; k < D; ++k) {
        const double g = gram[(size_t)k * n + (size_t)k];
        if (!(g != g || g == inf)) R.push_back(k);
    }
    const size_t r = R.size();
    std::vector<double> sc(n, inf);
    std::vector<int> sel(n, 0);
    std::vector<double> C(r * r), rho(r), u(r), t(r);
    if (r > 0) {  // rule 3
        double mu = 0.0;
        for (size_t a = 0; a < r; ++a) {
            double acc = 0.0;
            for (size_t b = 0; b < r; ++b) acc = add_r(acc, gram[(size_t)R[a] * n + (size_t)R[b]]);
            rho[a] = div_r(acc, (double)r);
            mu = add_r(mu, rho[a]);
        }
        mu = div_r(mu, (double)r);
        for (size_t a = 0; a < r; ++a)
            for (size_t b = 0; b < r; ++b)
                C[a * r + b] = add_r(add_r(add_r(gram[(size_t)R[a] * n + (size_t)R[b]], -rho[a]), -rho[b]), mu);
        size_t star = 0;  // rule 4
        for (size_t a = 1; a < r; ++a)
            if (C[a * r + a] > C[star * r + star]) star = a;
        const auto times_c = [&]() {  // t = C u
            for (size_t k = 0; k < r; ++k) {
                double acc = 0.0;
                for (size_t b = 0; b < r; ++b) acc = add_r(acc, mul_r(C[k * r + b], u[b]));
                t[k] = acc;
            }
        };
        if (C[star * r + star] > 0.0) {
            for (size_t b = 0; b < r; ++b) u[b] = C[b * r + star];
            for (int it = 0; it < iters; ++it) {  // rule 5
                times_c();
                double M = 0.0;
                bool nan = false;
                for (size_t k = 0; k < r; ++k) {
                    const double a = std::fabs(t[k]);
                    if (a != a) nan = true;
                    if (a > M) M = a;
                }
                if (nan || M == 0.0 || M == inf) break;
                for (size_t k = 0; k < r; ++k) u[k] = div_r(t[k], M);
            }
            times_c();  // rule 6
            for (size_t k = 0; k < r; ++k) sc[(size_t)R[k]] = mul_r(t[k], t[k]);
        } else {
            for (size_t k = 0; k < r; ++k) sc[(size_t)R[k]] = 0.0;
        }
        // rule 7: the q largest (s_k, k) go; a NaN score counts as +inf
        const int q = std::max(0, std::min(drop - (D - (int)r), (int)r - 1));
        std::vector<int> order(R);
        auto key = [&](int k) { return sc[(size_t)k] != sc[(size_t)k] ? inf : sc[(size_t)k]; };
        std::sort(order.begin(), order.end(), [&](int a, int b) { return key(a) != key(b) ? key(a) > key(b) : a > b; });
        for (int k : R) sel[(size_t)k] = 1;
        for (int i = 0; i < q; ++i) sel[(size_t)order[(size_t)i]] = 0;
    }
    int ns = 0;
    for (int k = 0; k < D; ++k) {
        if (scores) scores[k] = sc[(size_t)k];
        if (selected) selected[k] = sel[(size_t)k];
        ns += sel[(size_t)k];
    }
    if (n_selected) *n_selected = ns;
}

// Enqueues the Gram pass on the current device: d_gram (D * D doubles) = the matrix of clients[0..D) (n > 0 elements
// of `in`) against ref (nullable); d_part: the partials scratch.  The vector form where every client and ref allow it
// (fa_split.h).
int gram_on(const fa::Tuning& tu, const void* const* clients, int D, size_t n, fa_dtype in, const float* ref, double* d_part,
            double* d_gram, hipStream_t s) {
    fa::Split sp = fa::split_at(clients[0], dsize(in), n);
    for (int k = 0; k < D; ++k) sp.require_input(clients[k]);
    if (ref) sp.require(ref, 4);
    const fa::ClientTable t = client_table(clients, nullptr, 0, D);
    FA_HIP(fa::launch_gram(t, D, in, ref, sp, d_part, d_gram, tu, s));
    return FA_OK;
}

// ------------------------------------------------------------------ geomed stage

// The refusals of T and nu, and of D clients when D > 0 (fa.h "Geomed stage"), naming the cause.
int check_geomed(int D, int iters, float nu) {
    if (iters < 0 || iters > FA_GEOMED_MAX_ITERS)
        return fail(FA_ERR_ARG, "geomed: iters = %d outside 0..%d (0 removes the stage)", iters, FA_GEOMED_MAX_ITERS);
    if (iters != 0 && (!finite_f(nu) || !(nu > 0.0f))) return fail(FA_ERR_ARG, "geomed: nu %g must be finite and > 0", (double)nu);
    if (iters != 0 && D > FA_GEOMED_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "geomed: D = %d clients (at most %d)", D, FA_GEOMED_MAX_CLIENTS);
    return FA_OK;
}

// Rules 3-4 of fa.h "Geomed stage": volatile keeps each step one rounded fp64 operation.  W is the mass of the owners
// that entered the round: every k with w_k > 0, whatever `included` says by now.  *objective (nullable) = sum_k
// (double)w_k N_k over the clients still included after rule 3.
void geomed_weights(const float* w, const double* sumsq, int* included, int D, float nu, float* w_out, double* objective) {
    volatile double W = 0.0, B = 0.0, obj = 0.0;
    std::vector<double> beta((size_t)D, 0.0);
    for (int k = 0; k < D; ++k) {
        if (!(w[k] > 0.0f)) {
            included[k] = 0;
            continue;
        }
        W = W + (double)w[k];
        if (!included[k]) continue;
        volatile double nrm = std::sqrt(sumsq[k]);
        const double N = nrm;
        if (N != N || N == HUGE_VAL) {
            included[k] = 0;
            continue;
        }
        volatile double term = (double)w[k] * N;
        obj = obj + term;
        const double floor_ = (double)nu;
        volatile double b = (double)w[k] / (floor_ > N ? floor_ : N);
        beta[(size_t)k] = b;
        B = B + b;
    }
    volatile double ratio = 0.0;
    bool plain = !(B > 0.0);
    if (!plain) {
        ratio = W / B;
        const double r = ratio;
        plain = r != r || r == HUGE_VAL || r == -HUGE_VAL;
    }
    for (int k = 0; k < D; ++k) {
        if (!included[k]) {
            w_out[k] = 0.0f;
        } else if (plain) {
            w_out[k] = w[k];
        } else {
            volatile double prod = beta[(size_t)k] * ratio;
            w_out[k] = (float)prod;
        }
    }
    if (objective) *objective = obj;
}

constexpr size_t kGeomedParts = 2 * kClipParts;  // the fused pass's partials: Q and B of every client

// Enqueues the fused pass on the current device: d_out[k] = Q_k and d_out[nc + k] = B_k of clients[0..nc) (n > 0
// elements of `in`) under the weights w, d_v (nullable, n fp32) = the chain; d_part: kGeomedParts doubles of scratch.
// The vector form where every client (and d_v) allows it (fa_split.h).
int geomed_pass_on(const fa::Tuning& tu, const void* const* clients, const float* w, int nc, size_t n, fa_dtype in,
                   float* d_v, double* d_part, double* d_out, hipStream_t s) {
    fa::Split sp = fa::split_at(clients[0], dsize(in), n);
    for (int k = 0; k < nc; ++k) sp.require_input(clients[k]);
    if (d_v) sp.require(d_v, 4);
    const fa::ClientTable t = client_table(clients, w, 0, nc);
    FA_HIP(fa::launch_geomed_pass(t, nc, in, d_v, sp, d_part, d_out, tu, s));
    return FA_OK;
}

// ------------------------------------------------------------------ Bulyan stage

// The refusals of f for D clients (fa.h "Bulyan stage"), naming the cause.
int check_bulyan(int D, int f) {
    if (D > FA_TRIMMED_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "bulyan: D = %d clients (at most %d)", D, FA_TRIMMED_MAX_CLIENTS);
    if (f < 0 || 4 * f + 3 > D)
        return fail(FA_ERR_ARG, "bulyan: f = %d does not fit D = %d clients (0 <= f and 4 f + 3 <= D)", f, D);
    return FA_OK;
}

// Rule 2 of fa.h "Bulyan stage" (D, f checked): order, pick_scores and selected hold D entries each, any may be
// null.  Every row is sorted once with its column indices; a round's score is the row's first entries that are
// still in R, which is the sorted row of rule 2 (equal values add to the same sum in either order).  volatile
// keeps each step one rounded fp64 add.
void bulyan_select(const double* dist, int D, int f, int* order, double* pick_scores, int* selected, int* n_selected) {
    const double inf = HUGE_VAL;
    const size_t n = (size_t)D;
    std::vector<std::vector<std::pair<double, int>>> rows(n);
    for (int k = 0; k < D; ++k) {
        auto& row = rows[(size_t)k];
        row.reserve(n - 1);
        for (int j = 0; j < D; ++j) {
            if (j == k) continue;
            const double q = dist[(size_t)k * n + (size_t)j];
            row.emplace_back(q != q ? inf : q, j);
        }
        std::stable_sort(row.begin(), row.end(),
                         [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
    }
    std::vector<char> in_r(n, 1);
    for (int k = 0; k < D; ++k) {
        if (order) order[k] = -1;
        if (pick_scores) pick_scores[k] = inf;
        if (selected) selected[k] = 0;
    }
    const int theta = D - 2 * f;
    int picked = 0;
    for (int left = D; picked < theta; --left) {
        const int take = std::min(std::max(1, left - f - 2), left - 1);
        int best = -1;
        double best_s = inf;
        for (int k = 0; k < D; ++k) {
            if (!in_r[(size_t)k]) continue;
            volatile double acc = 0.0;
            int got = 0;
            for (const auto& e : rows[(size_t)k]) {
                if (got == take) break;
                if (!in_r[(size_t)e.second]) continue;
                acc = acc + e.first;
                ++got;
            }
            const double s = acc;
            const double key = s != s ? inf : s;  // a NaN score (only from a matrix holding -inf) counts as +inf
            if (best < 0 || key < best_s) {
                best = k;
                best_s = key;
            }
        }
        if (!(best_s < inf)) break;  // +inf is never picked, nor anything after it
        if (order) order[picked] = best;
        if (pick_scores) pick_scores[picked] = best_s;
        if (selected) selected[best] = 1;
        in_r[(size_t)best] = 0;
        ++picked;
    }
    if (n_selected) *n_selected = picked;
}

// Enqueues the centred mean (rule 4) on the current device: nc clients (n > 0 elements of `in`) -> dst.
int centered_on(const fa::Tuning& tu, const void* const* clients, int nc, size_t n, fa_dtype in, void* dst, fa_dtype out,
                int keep, hipStream_t s) {
    const size_t si = dsize(in), so = dsize(out);
    if (int rc = check_clients(clients, nc, si, "client")) return rc;
    if (!dst) return fail(FA_ERR_ARG, "output pointer is null");
    if (!aligned(dst, so)) return fail(FA_ERR_ALIGN, "output not %zu-byte aligned", so);
    fa::Split sp = fa::split_at(clients[0], si, n);
    for (int k = 0; k < nc; ++k) sp.require_input(clients[k]);
    sp.require(dst, so);
    const fa::ClientTable t = client_table(clients, nullptr, 0, nc);
    FA_HIP(fa::launch_centered(t, nc, in, out, keep, dst, sp, tu, s));
    return FA_OK;
}

// The body of the two raw device entries (arguments checked): one measure pass, enqueue(call, d_part, d_out) ->
// FA_*, on the context's scratch, or without a context on scratch of its own, freed before the return; its
// `outs` results into h_out after the wait for the stream, which follows whatever was enqueued (MeasureScratch).
template <typename Enqueue>
int measure_device(fa_ctx* ctx, int gpu, void* hip_stream, size_t outs, size_t parts, const char* stage, double* h_out,
                   Enqueue enqueue) {
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    MeasureScratch own;
    MeasureScratch& m = ctx ? ctx->gpu[(size_t)gpu].measure : own;
    int rc = ensure_measure_scratch(m, outs, parts, stage);
    hipError_t e = hipSuccess;
    if (!rc) {
        rc = enqueue(c, m.dev + m.outs, m.dev);
        if (!rc) e = hipMemcpyAsync(m.host, m.dev, outs * sizeof(double), hipMemcpyDeviceToHost, c.s);
        const hipError_t es = hipStreamSynchronize(c.s);
        if (e == hipSuccess) e = es;
        if (!rc && e == hipSuccess) std::copy(m.host, m.host + outs, h_out);
    }
    if (!ctx) free_measure_scratch(own);
    if (rc) return rc;
    FA_HIP(e);
    return FA_OK;
}

// The size of a stage's fp32 array over GPU g's elements.
inline size_t f32_bytes(const Part& p, size_t g) { return std::max<size_t>(16, p.cnt[g] * 4); }

// The fp32 aggregate buffer of a 16-bit part: wanted while it has a server-optimizer or a noise stage.
inline bool wants_oavg(const Part& p) { return p.out != FA_F32 && (p.opt.on() || p.noise.on()); }
void drop_oavg_if_unused(fa_ctx* ctx, Part& p) {
    if (!wants_oavg(p)) p.oavg.free(ctx->gpu);
}
// Allocates it if it is wanted and not there (`stage` names the caller in the message).
int ensure_oavg(fa_ctx* ctx, Part& p, const char* stage) {
    if (!wants_oavg(p) || p.oavg) return FA_OK;
    const int g = p.oavg.alloc(ctx->gpu, [&](size_t i) { return f32_bytes(p, i); });
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "%s: aggregate buffer alloc of %zu B failed on GPU %zu", stage, f32_bytes(p, (size_t)g), (size_t)g);
}

// What a stage holds on the devices goes (hipFree waits for the device's pending work) with its state and report: the
// optimizer's master, the clip reference, the MX8 shadows (the part takes full receipts only), `sent` and the codes.
void free_opt(fa_ctx* ctx, Part& p) {
    for (DevArrays* a : {&p.opt.x, &p.opt.m, &p.opt.v}) a->free(ctx->gpu);
    p.opt = OptStage{};
    drop_oavg_if_unused(ctx, p);
}
void free_clip(fa_ctx* ctx, Part& p) {
    for (DevArrays* a : {&p.clip.ref, &p.clip.init}) a->free(ctx->gpu);
    p.clip = ClipStage{};
}
void free_mx8(fa_ctx* ctx, Part& p) {
    p.mx8.buf.free(ctx->gpu);
    p.mx8.sparse.free(ctx->gpu);
    p.mx8.plan.free(ctx->gpu);
    p.mx8.factors.free(ctx->gpu);
    p.mx8.rot.free(ctx->gpu);
    p.mx8 = Mx8Stage{};
}
void free_reply(fa_ctx* ctx, Part& p) {
    for (DevArrays* a : {&p.reply.sent, &p.reply.codes}) a->free(ctx->gpu);
    p.reply = ReplyStage{};
}
void free_secagg(fa_ctx* ctx, Part& p) {
    p.secagg.dev.free(ctx->gpu);
    p.secagg = SecaggStage{};
}
void free_sign(fa_ctx* ctx, Part& p) {
    for (DevArrays* a : {&p.sign.buf, &p.sign.planes}) a->free(ctx->gpu);
    p.sign = SignStage{};
}
void free_sparse(fa_ctx* ctx, Part& p) {
    for (DevArrays* a : {&p.sparse.buf, &p.sparse.work}) a->free(ctx->gpu);
    p.sparse = SparseStage{};
}
void free_mx8sum(fa_ctx* ctx, Part& p) {
    p.mx8sum.buf.free(ctx->gpu);
    p.mx8sum = Mx8SumStage{};
}
void free_lrsum(fa_ctx* ctx, Part& p) {
    for (DevArrays* a : {&p.lrsum.plan, &p.lrsum.factors}) a->free(ctx->gpu);
    p.lrsum = LowrankSumStage{};
}
void free_rot1sum(fa_ctx* ctx, Part& p) {
    p.rot1sum.buf.free(ctx->gpu);
    p.rot1sum = Rot1SumStage{};
}
void free_stages(fa_ctx* ctx, Part& p) {
    p.noise = NoiseStage{};
    free_secagg(ctx, p);
    free_sign(ctx, p);
    free_sparse(ctx, p);
    free_mx8sum(ctx, p);
    free_lrsum(ctx, p);
    free_rot1sum(ctx, p);
    free_mx8(ctx, p);
    free_reply(ctx, p);
    free_opt(ctx, p);
    free_clip(ctx, p);
}

// A stage's measure pass over part p (range layout).  On every GPU with elements, after its H2D copies:
// launch(g, j, clients, cnt, d_part, d_out, stream) -> FA_* enqueues the pass of piece j, in order, its `outs`
// fp64 results into d_out (d_part: `parts` partials of scratch), then one D2H brings all the pieces' results.
// Then, per GPU in order, one wait and each piece's results into acc[0, outs), zeroed by the caller: one rounded
// fp64 add per element, in GPU order, then piece order (fa.h).  An error ends the enqueuing, not the waits:
// every GPU enqueued on is waited for (MeasureScratch).
template <typename Launch>
int measure_pass(fa_ctx* ctx, Part& p, hipStream_t s, size_t outs, size_t parts, const char* stage, double* acc,
                 Launch launch) {
    std::vector<const void*> ptrs;
    const auto enqueue = [&](int g) -> int {
        MeasureScratch& m = ctx->gpu[(size_t)g].measure;
        hipStream_t st = s ? s : ctx->gpu[(size_t)g].compute;
        const size_t np = (size_t)p.npiece[(size_t)g];
        int rc = wait_copies(ctx, g, st);
        if (rc || (rc = ensure_measure_scratch(m, np * outs, parts, stage))) return rc;
        for (size_t j = 0; j < np; ++j)
            if ((rc = launch(g, (int)j, piece_ptrs(p, g, (int)j, 0, p.D, ptrs), piece_cnt(p, g, (int)j), m.dev + m.outs,
                             m.dev + j * outs, st)))
                return rc;
        FA_HIP(hipMemcpyAsync(m.host, m.dev, np * outs * sizeof(double), hipMemcpyDeviceToHost, st));
        return FA_OK;
    };
    int rc = FA_OK, tried = 0;  // GPUs [0, tried) may have work of this pass in flight
    for (; !rc && tried < ctx->G; ++tried) {
        if (p.cnt[(size_t)tried] == 0) continue;
        DeviceGuard dg(ctx->gpu[(size_t)tried].dev);
        rc = enqueue(tried);
    }
    for (int g = 0; g < tried; ++g) {
        if (p.cnt[(size_t)g] == 0) continue;
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        const hipError_t e = hipStreamSynchronize(s ? s : r.compute);
        if (rc) continue;
        if (e != hipSuccess) {
            rc = fail(FA_ERR_HIP, "hipStreamSynchronize(s ? s : r.compute): %s (%s:%d)", hipGetErrorString(e), __FILE__,
                      __LINE__);
            continue;
        }
        for (size_t j = 0; j < (size_t)p.npiece[(size_t)g]; ++j)
            for (size_t i = 0; i < outs; ++i) {
                volatile double q = acc[i] + r.measure.host[j * outs + i];
                acc[i] = q;
            }
    }
    return rc;
}

// Rules 1-3 for part p (range layout, a reference present): the norm pass (measure_pass), then the host
// arithmetic.  Leaves the round's report in the part.
int clip_plan(fa_ctx* ctx, Part& p, const float* w, hipStream_t s, SubsetPlan* plan) {
    const size_t D = (size_t)p.D;
    std::fill(p.clip.q.begin(), p.clip.q.end(), 0.0);
    if (int rc = measure_pass(ctx, p, s, D, kClipParts, "clip: norm-pass", p.clip.q.data(),
                              [&](int g, int j, const void* const* clients, size_t cnt, double* d_part, double* d_out,
                                  hipStream_t st) {
                                  return clip_sumsq_on(ctx->tuning.tu, clients, p.D, cnt, p.in,
                                                       p.clip.ref.at<float>((size_t)g) + piece_lo(p, g, j), d_part, d_out, st);
                              }))
        return rc;
    double W = 0.0, Wp = 0.0;
    p.clip.n = 0;
    for (size_t k = 0; k < D; ++k) {
        int ex = 0;
        const float sc = clip_scale(p.clip.q[k], p.clip.cfg.max_norm, &ex);
        p.clip.s[k] = sc;
        p.clip.in[k] = ex ? 0 : 1;
        W += (double)w[k];
        if (ex) continue;
        if (sc < 1.0f) ++p.clip.n;
        volatile float prod = w[k] * sc;  // one rounded fp32 product
        const float wk = prod;
        Wp += (double)wk;
        plan->inc.push_back((int)k);
        plan->w.push_back(wk);
    }
    volatile double rest = W - Wp;
    plan->c0 = (float)rest;
    return FA_OK;
}

// The chain of a stage's plan for piece j of GPU g (the current device), into dst (dtype odt): over the plan's
// clients (clip rule 4, Krum rule 5), with c0 != 0 the clip reference as its first term.  An f32 part passes g
// as the chain's first client with weight c0; a 16-bit part first writes fmaf(c0, g, +0) into its fp32 buffer
// (a one-client f32 chain) and continues from it.  Only then are p.cref and p.cinit touched: a Krum part has
// neither.
int subset_chain(fa_ctx* ctx, Part& p, int g, int j, const SubsetPlan& plan, void* dst, fa_dtype odt, hipStream_t st) {
    const size_t lo = piece_lo(p, g, j), cnt = piece_cnt(p, g, j);
    if (cnt == 0) return FA_OK;
    const fa::Tuning& tu = ctx->tuning.tu;
    const bool lead = plan.c0 != 0.0f;
    const void* ref = lead ? p.clip.ref.at<float>((size_t)g) + lo : nullptr;
    if (plan.inc.empty()) {  // the first term alone, +0 without one
        if (lead) return reduce_on(ctx, g, tu, &ref, &plan.c0, 1, cnt, FA_F32, dst, odt, FA_FEDAVG, 0.0f, nullptr, st);
        FA_HIP(hipMemsetAsync(dst, 0, cnt * dsize(odt), st));
        return FA_OK;
    }
    std::vector<const void*> ptrs;
    std::vector<float> ws;
    const float* init = nullptr;
    if (lead && p.in == FA_F32) {
        ptrs.push_back(ref);
        ws.push_back(plan.c0);
    } else if (lead) {
        float* first = p.clip.init.at<float>((size_t)g) + lo;
        if (int rc = reduce_on(ctx, g, tu, &ref, &plan.c0, 1, cnt, FA_F32, first, FA_F32, FA_FEDAVG, 0.0f, nullptr, st))
            return rc;
        init = first;
    }
    for (size_t i = 0; i < plan.inc.size(); ++i) {
        ptrs.push_back(piece_ptr(p, g, plan.inc[i], j));
        ws.push_back(plan.w[i]);
    }
    return reduce_on(ctx, g, tu, ptrs.data(), ws.data(), (int)ptrs.size(), cnt, p.in, dst, odt, FA_FEDAVG, 0.0f, init, st);
}

// The buffers of a reply part, allocated once: per GPU `sent` (cnt elements of the out dtype) and the codes (q: cnt
// bytes, then from eoff[g] on the scale bytes of the blocks the range touches).  On failure the part keeps its stage.
int ensure_reply_buf(fa_ctx* ctx, Part& p) {
    ReplyStage& s = p.reply;
    if (s.sent) return FA_OK;
    s.eoff.clear();
    for (size_t cnt : p.cnt) s.eoff.push_back((cnt + 15) / 16 * 16);
    const auto sbytes = [&](size_t g) { return std::max<size_t>(256, p.cnt[g] * dsize(p.out)); };
    const auto cbytes = [&](size_t g) {
        const size_t scales = p.cnt[g] ? ((p.off[g] + p.cnt[g] - 1) >> 5) - (p.off[g] >> 5) + 1 : 0;
        return std::max<size_t>(256, s.eoff[g] + scales);
    };
    int g = s.sent.alloc(ctx->gpu, sbytes);
    if (g < 0 && (g = s.codes.alloc(ctx->gpu, cbytes)) >= 0) s.sent.free(ctx->gpu);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "mx8 reply: alloc of %zu + %zu B failed on GPU %zu", sbytes((size_t)g), cbytes((size_t)g), (size_t)g);
}

// The reply stage on GPU g (fa.h "MX8 replies", rules 2-5), after everything else of the reducing call: the output
// holds y.  Without `sent` the round is the bootstrap, sent := y; else one fused pass writes the codes, g' into
// the output and g' into `sent`.  Range shards are cut at multiples of 64 elements (kShardUnit), so no block of 32
// lies in two GPUs' ranges and rule 6's exchange of partial scales never arises here; a layout that cut
// elsewhere would have to run fa_mx8_encode_device's two scale modes around a host wait, and is refused.
int reply_stage(fa_ctx* ctx, Part& p, int g, hipStream_t st) {
    if (int rc = ensure_reply_buf(ctx, p)) return rc;
    const size_t cnt = p.cnt[(size_t)g], off = p.off[(size_t)g];
    if (cnt == 0) return FA_OK;
    if (off % FA_MX8_BLOCK != 0)
        return fail(FA_ERR_STATE, "mx8 reply: part %d: the range of GPU %d starts at element %zu, inside a block", p.id, g, off);
    char* sent = p.reply.sent.at((size_t)g);
    if (!p.reply.has_sent) {
        FA_HIP(hipMemcpyAsync(sent, p.dout[(size_t)g], cnt * dsize(p.out), hipMemcpyDeviceToDevice, st));
        return FA_OK;
    }
    char* q = p.reply.codes.at((size_t)g);
    FA_HIP(fa::launch_mx8_encode(p.dout[(size_t)g], sent, p.out, (uint64_t)off, (int64_t)cnt, reinterpret_cast<int8_t*>(q),
                                 reinterpret_cast<uint8_t*>(q + p.reply.eoff[(size_t)g]), p.dout[(size_t)g], sent,
                                 fa::kMx8EncFused, st));
    return FA_OK;
}

// After reply_stage ran on every GPU: a round with `sent` left codes, the bootstrap left `sent`.
void reply_round_done(Part& p) {
    p.reply.has_codes = p.reply.has_sent;
    p.reply.has_sent = true;
    p.reply.counted = !p.reply.has_codes;
    p.reply.nan = 0;
}

// Rule 6 of the clip stage for piece j of GPU g: the reference := the output just written, widened to fp32.
int clip_take_reference(Part& p, int g, int j, hipStream_t st) {
    const size_t lo = piece_lo(p, g, j), cnt = piece_cnt(p, g, j);
    if (cnt == 0) return FA_OK;
    const char* out = static_cast<const char*>(p.dout[(size_t)g]) + lo * dsize(p.out);
    float* ref = p.clip.ref.at<float>((size_t)g) + lo;
    if (p.out == FA_F32) FA_HIP(hipMemcpyAsync(ref, out, cnt * 4, hipMemcpyDeviceToDevice, st));
    else FA_HIP(fa::launch_clip_widen(out, p.out, ref, (int64_t)cnt, st));
    return FA_OK;
}

// Rules 1-4 for part p (range layout): the distance pass (measure_pass), then the host arithmetic.  Leaves the
// round's report in the part.
int krum_plan(fa_ctx* ctx, Part& p, const float* w, hipStream_t s, SubsetPlan* plan) {
    const size_t D = (size_t)p.D;
    p.krum.q.assign(D * D, 0.0);
    if (int rc = measure_pass(ctx, p, s, D * D, krum_parts(p.D), "krum: distance-pass", p.krum.q.data(),
                              [&](int, int, const void* const* clients, size_t cnt, double* d_part, double* d_out,
                                  hipStream_t st) {
                                  return pairdist_on(ctx->tuning.tu, clients, p.D, cnt, p.in, d_part, d_out, st);
                              }))
        return rc;
    p.krum.s.assign(D, 0.0);
    p.krum.sel.assign(D, 0);
    krum_select(p.krum.q.data(), p.D, p.krum.cfg.f, p.krum.cfg.m, p.krum.s.data(), p.krum.sel.data(), &p.krum.n);
    std::vector<float> wp(D);
    krum_weights(w, p.krum.sel.data(), p.D, wp.data());
    for (size_t k = 0; k < D; ++k)
        if (p.krum.sel[k]) {
            plan->inc.push_back((int)k);
            plan->w.push_back(wp[k]);
        }
    p.krum.reported = true;
    return FA_OK;
}

// Rules 1-8 of the DnC stage for part p (range layout): the Gram pass (measure_pass, no reference), then the host
// arithmetic and the Krum stage's weights.  Leaves the round's report in the part.
int dnc_plan(fa_ctx* ctx, Part& p, const float* w, hipStream_t s, SubsetPlan* plan) {
    const size_t D = (size_t)p.D;
    p.dnc.q.assign(D * D, 0.0);
    if (int rc = measure_pass(ctx, p, s, D * D, gram_parts(p.D), "dnc: gram-pass", p.dnc.q.data(),
                              [&](int, int, const void* const* clients, size_t cnt, double* d_part, double* d_out,
                                  hipStream_t st) {
                                  return gram_on(ctx->tuning.tu, clients, p.D, cnt, p.in, nullptr, d_part, d_out, st);
                              }))
        return rc;
    p.dnc.s.assign(D, 0.0);
    p.dnc.sel.assign(D, 0);
    dnc_select(p.dnc.q.data(), p.D, p.dnc.cfg.drop, p.dnc.cfg.iters, p.dnc.s.data(), p.dnc.sel.data(), &p.dnc.n);
    std::vector<float> wp(D);
    krum_weights(w, p.dnc.sel.data(), p.D, wp.data());
    for (size_t k = 0; k < D; ++k)
        if (p.dnc.sel[k]) {
            plan->inc.push_back((int)k);
            plan->w.push_back(wp[k]);
        }
    p.dnc.reported = true;
    return FA_OK;
}

// Rules 0-4 for part p (range layout): T fused passes (measure_pass over the included clients alone, 2 m results: Q
// then B), each followed by the host arithmetic; a pass that finds a non-finite bucket is void and repeated without
// its owner.  The plan is the final chain's: the included clients and alpha^T.  Leaves the round's trace in the part.
int geomed_plan(fa_ctx* ctx, Part& p, const float* w, hipStream_t s, SubsetPlan* plan) {
    const size_t D = (size_t)p.D;
    const int T = p.geomed.cfg.iters;
    p.geomed.q.assign((size_t)T * D, 0.0);
    p.geomed.w.assign((size_t)(T + 1) * D, 0.0f);
    p.geomed.obj.assign((size_t)T, 0.0);
    p.geomed.in.assign(D, 0);
    p.geomed.passes = 0;
    std::vector<int>& inc = p.geomed.in;
    std::vector<float> alpha(D, 0.0f);
    for (size_t k = 0; k < D; ++k) {
        inc[k] = w[k] > 0.0f ? 1 : 0;
        if (inc[k]) alpha[k] = w[k];
    }
    std::vector<int> idx;
    std::vector<float> wsub;
    std::vector<const void*> sub;
    std::vector<double> res;
    const double* last_q = nullptr;  // the last valid pass's row
    int t = 0;
    while (t < T) {
        idx.clear();
        wsub.clear();
        for (size_t k = 0; k < D; ++k)
            if (inc[k]) {
                idx.push_back((int)k);
                wsub.push_back(alpha[k]);
            }
        const size_t m = idx.size();
        if (m == 0) break;  // nobody left: the aggregate is +0
        res.assign(2 * m, 0.0);
        if (int rc = measure_pass(ctx, p, s, 2 * m, kGeomedParts, "geomed: fused pass", res.data(),
                                  [&](int, int, const void* const* clients, size_t cnt, double* d_part, double* d_out,
                                      hipStream_t st) {
                                      sub.resize(m);
                                      for (size_t i = 0; i < m; ++i) sub[i] = clients[idx[i]];
                                      return geomed_pass_on(ctx->tuning.tu, sub.data(), wsub.data(), (int)m, cnt, p.in, nullptr,
                                                            d_part, d_out, st);
                                  }))
            return rc;
        bool removed = false;
        for (size_t i = 0; i < m; ++i)
            if (res[m + i] > 0.0) {  // rule 2: a non-finite bucket poisons v; the pass is void
                inc[(size_t)idx[i]] = 0;
                removed = true;
            }
        if (removed) {
            for (size_t k = 0; k < D; ++k) alpha[k] = inc[k] ? w[k] : 0.0f;
            if (last_q) geomed_weights(w, last_q, inc.data(), p.D, p.geomed.cfg.nu, alpha.data(), nullptr);
            continue;
        }
        double* qrow = &p.geomed.q[(size_t)t * D];
        for (size_t i = 0; i < m; ++i) qrow[(size_t)idx[i]] = res[i];
        std::copy(alpha.begin(), alpha.end(), p.geomed.w.begin() + (ptrdiff_t)((size_t)t * D));
        geomed_weights(w, qrow, inc.data(), p.D, p.geomed.cfg.nu, alpha.data(), &p.geomed.obj[(size_t)t]);
        last_q = qrow;
        p.geomed.passes = ++t;
    }
    for (size_t k = 0; k < D; ++k)
        if (!inc[k]) alpha[k] = 0.0f;
    std::copy(alpha.begin(), alpha.end(), p.geomed.w.begin() + (ptrdiff_t)((size_t)p.geomed.passes * D));
    for (size_t k = 0; k < D; ++k)
        if (inc[k]) {
            plan->inc.push_back((int)k);
            plan->w.push_back(alpha[k]);
        }
    p.geomed.reported = true;
    return FA_OK;
}

// Rules 1-2 of the Bulyan stage for part p (range layout): the distance pass (measure_pass), then the iterated
// selection.  The plan's clients are the picks in ascending client order; its weights stay empty (the rule has
// none).  Leaves the round's report in the part.
int bulyan_plan(fa_ctx* ctx, Part& p, hipStream_t s, SubsetPlan* plan) {
    const size_t D = (size_t)p.D;
    p.bulyan.q.assign(D * D, 0.0);
    if (int rc = measure_pass(ctx, p, s, D * D, krum_parts(p.D), "bulyan: distance-pass", p.bulyan.q.data(),
                              [&](int, int, const void* const* clients, size_t cnt, double* d_part, double* d_out,
                                  hipStream_t st) {
                                  return pairdist_on(ctx->tuning.tu, clients, p.D, cnt, p.in, d_part, d_out, st);
                              }))
        return rc;
    p.bulyan.s.assign(D, 0.0);
    p.bulyan.order.assign(D, -1);
    p.bulyan.sel.assign(D, 0);
    bulyan_select(p.bulyan.q.data(), p.D, p.bulyan.cfg.f, p.bulyan.order.data(), p.bulyan.s.data(), p.bulyan.sel.data(),
                  &p.bulyan.n);
    for (size_t k = 0; k < D; ++k)
        if (p.bulyan.sel[k]) plan->inc.push_back((int)k);
    p.bulyan.reported = true;
    return FA_OK;
}

// Rule 3 for piece j of GPU g (the current device), into dst (dtype odt): the centred mean over the plan's
// clients keeping max(1, theta' - 2f) of them, +0 when nobody was picked.
int bulyan_piece(fa_ctx* ctx, Part& p, int g, int j, const SubsetPlan& plan, void* dst, fa_dtype odt, hipStream_t st) {
    const size_t cnt = piece_cnt(p, g, j);
    if (cnt == 0) return FA_OK;
    if (plan.inc.empty()) {
        FA_HIP(hipMemsetAsync(dst, 0, cnt * dsize(odt), st));
        return FA_OK;
    }
    std::vector<const void*> ptrs;
    for (int k : plan.inc) ptrs.push_back(piece_ptr(p, g, k, j));
    const int nc = (int)ptrs.size();
    return centered_on(ctx->tuning.tu, ptrs.data(), nc, cnt, p.in, dst, odt, std::max(1, nc - 2 * p.bulyan.cfg.f), st);
}

// ------------------------------------------------------------------ secagg stage

constexpr uint64_t kSecaggMaxIndex = (uint64_t)1 << 36;  // idx0 + n: the block counter i >> 4 is a uint32

// The refusals shared by fa_set_secagg and fa_secagg_unmask_device.
int check_secagg_scale(float scale) {
    if (!finite_f(scale) || !(scale > 0.0f)) return fail(FA_ERR_ARG, "secagg: scale %g must be finite and > 0", (double)scale);
    return FA_OK;
}
int check_secagg_range(uint64_t idx0, size_t n) {
    if (idx0 > kSecaggMaxIndex || (uint64_t)n > kSecaggMaxIndex - idx0)
        return fail(FA_ERR_ARG, "secagg: idx0 + n beyond 2^36 (the ChaCha20 block counter has 32 bits)");
    return FA_OK;
}
int check_secagg_terms(int T, const uint32_t* keys, const uint32_t* nonces, const int* signs) {
    if (T < 0 || T > FA_SECAGG_MAX_TERMS) return fail(FA_ERR_ARG, "secagg: T = %d terms outside 0..%d", T, FA_SECAGG_MAX_TERMS);
    if (T > 0 && (!keys || !nonces || !signs))
        return fail(FA_ERR_ARG, "secagg: %s is null", !keys ? "keys" : !nonces ? "nonces" : "signs");
    for (int t = 0; t < T; ++t)
        if (signs[t] != 1 && signs[t] != -1) return fail(FA_ERR_ARG, "secagg: sign %d of term %d is neither +1 nor -1", signs[t], t);
    return FA_OK;
}

// The unmasking on the current device: D buckets of n uint32 words that are bucket elements idx0 .., the T terms of
// the device table d_tab -> dst (dtype odt).  D beyond kMaxClients: passes that continue the uint32 sums, in dst
// itself for an f32 output, else in the context's scratch; the terms go into the last one.
int secagg_on(fa_ctx* ctx, int g, const fa::Tuning& tu, const void* const* clients, int D, size_t n, uint64_t idx0,
              const uint32_t* d_tab, int T, int npos, uint32_t cnet, float scale, void* dst, fa_dtype odt, int form,
              hipStream_t s) {
    if (n == 0) return FA_OK;
    const size_t so = dsize(odt);
    if (int rc = check_clients(clients, D, 4, "client")) return rc;
    if (!dst) return fail(FA_ERR_ARG, "output pointer is null");
    if (!aligned(dst, so)) return fail(FA_ERR_ALIGN, "output not %zu-byte aligned", so);
    fa::Split sp = fa::secagg_split(clients[0], idx0, n);
    for (int k = 0; k < D; ++k) sp.require_input(clients[k]);
    sp.require(dst, so);
    const int passes = (D + fa::kMaxClients - 1) / fa::kMaxClients;
    uint32_t* acc = nullptr;
    if (passes > 1) {
        if (odt == FA_F32) {
            acc = static_cast<uint32_t*>(dst);
        } else {
            if (!ctx) return fail(FA_ERR_ARG, "%s output with D > %d needs a ctx for scratch", fa::dtype_name(odt), fa::kMaxClients);
            if (int rc = ensure_scratch(ctx, g, n * 4)) return rc;
            acc = static_cast<uint32_t*>(ctx->gpu[(size_t)g].scratch);
            sp.require(acc, 4);
        }
    }
    for (int p = 0; p < passes; ++p) {
        const int k0 = p * fa::kMaxClients, nc = std::min(fa::kMaxClients, D - k0);
        const fa::ClientTable t = client_table(clients, nullptr, k0, nc);
        const bool last = p == passes - 1;
        FA_HIP(fa::launch_secagg(t, nc, d_tab, T, npos, cnet, p ? acc : nullptr, last ? dst : (void*)acc, odt, !last, scale,
                                 idx0, sp, form, tu, s));
    }
    return FA_OK;
}

// The device tables of a secagg part, allocated once: room for FA_SECAGG_MAX_TERMS terms per GPU.
int ensure_secagg_tab(fa_ctx* ctx, Part& p) {
    if (p.secagg.dev) return FA_OK;
    const size_t bytes = fa::secagg_table_words(FA_SECAGG_MAX_TERMS) * 4;
    const int g = p.secagg.dev.alloc(ctx->gpu, [&](size_t) { return bytes; });
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "secagg: term table alloc of %zu B failed on GPU %zu", bytes, (size_t)g);
}

// The round's terms onto every GPU that holds elements, on the stream its pieces will run on and after the part's
// last reducing call, which may have read the table on another stream.
int secagg_round_begin(fa_ctx* ctx, Part& p, hipStream_t s) {
    SecaggStage& sa = p.secagg;
    if (!sa.have)
        return fail(FA_ERR_STATE, "secagg: part %d has no terms for this round (fa_secagg_set_terms before every reducing "
                                  "call; T = 0 is set explicitly)", p.id);
    if (int rc = ensure_secagg_tab(ctx, p)) return rc;
    for (int g = 0; g < ctx->G; ++g) {
        if (p.cnt[(size_t)g] == 0) continue;
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        hipStream_t st = s ? s : r.compute;
        if (hipStream_t ds = p.done_stream[(size_t)g]; ds && ds != st) {
            FA_HIP(hipEventRecord(p.done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(st, p.done[(size_t)g], 0));
        }
        FA_HIP(hipMemcpyAsync(sa.dev.at((size_t)g), sa.tab.data(), sa.tab.size() * 4, hipMemcpyHostToDevice, st));
    }
    return FA_OK;
}

// Rules 2-4 for piece j of GPU g (the current device), into dst (dtype odt): every client of the part, the round's terms.
int secagg_piece(fa_ctx* ctx, Part& p, int g, int j, std::vector<const void*>& ptrs, void* dst, fa_dtype odt, hipStream_t st) {
    const SecaggStage& sa = p.secagg;
    return secagg_on(ctx, g, ctx->tuning.tu, piece_ptrs(p, g, j, 0, p.D, ptrs), p.D, piece_cnt(p, g, j),
                     (uint64_t)(p.off[(size_t)g] + piece_lo(p, g, j)), sa.dev.at<uint32_t>((size_t)g), sa.T, sa.npos, sa.cnet,
                     sa.cfg.scale, dst, odt, -1, st);
}

// ------------------------------------------------------------------ sign-vote stage

int mx8_h2d(GpuRes& r, char* dev, const char* src, size_t bytes, bool pinned);  // below, with the receipts

// The refusals shared by fa_set_sign, fa_sign_vote_device and fa_sign_vote_host.
int check_sign_params(float eta, int rule, int margin, bool planes) {
    if (!finite_f(eta) || !(eta > 0.0f)) return fail(FA_ERR_ARG, "sign: eta %g must be finite and > 0", (double)eta);
    if (rule != FA_SIGN_MAJORITY && rule != FA_SIGN_MEAN) return fail(FA_ERR_ARG, "sign: rule %d is neither FA_SIGN_MAJORITY nor FA_SIGN_MEAN", rule);
    if (margin < 1 || margin > FA_SIGN_MAX_CLIENTS) return fail(FA_ERR_ARG, "sign: margin %d outside 1 .. D", margin);
    if (planes && rule == FA_SIGN_MEAN) return fail(FA_ERR_STATE, "sign: the vote planes exist under the majority rule only");
    return FA_OK;
}
int check_sign_clients(int D, int margin) {
    if (D < 1 || D > FA_SIGN_MAX_CLIENTS) return fail(FA_ERR_ARG, "sign: D = %d clients outside 1 .. %d", D, FA_SIGN_MAX_CLIENTS);
    if (margin > D) return fail(FA_ERR_ARG, "sign: margin %d outside 1 .. D = %d", margin, D);
    return FA_OK;
}

// The words of a range of cnt elements that starts at a multiple of 32, and the bytes of a shadow or a plane of it.
inline size_t sign_words(size_t cnt) { return (cnt + 31) / 32; }
inline size_t sign_stride(size_t cnt) { return (sign_words(cnt) * 4 + 255) / 256 * 256; }

// The sign shadows of a part, allocated once: per GPU held x stride bytes.  On failure the part keeps the stage.
int ensure_sign_buf(fa_ctx* ctx, Part& p) {
    SignStage& s = p.sign;
    if (s.buf) return FA_OK;
    s.stride.clear();
    for (size_t g = 0; g < (size_t)ctx->G; ++g) s.stride.push_back(sign_stride(p.cnt[g]));
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.stride[g]); };
    const int g = s.buf.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "sign: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

int submit_sign_impl(fa_ctx* ctx, int part_id, int slot, const uint32_t* bits, int flags) {
    Trace tr("fa_submit_sign part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~FA_HOST_PINNED) return fail(FA_ERR_ARG, "sign: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    if (!p->sign.on()) return fail(FA_ERR_STATE, "sign: part %d has no sign-vote stage (fa_set_sign)", part_id);
    if (p->n > 0 && !bits) return fail(FA_ERR_ARG, "sign: bits is null");
    if ((rc = ensure_sign_buf(ctx, *p))) return rc;
    const bool pinned = (flags & FA_HOST_PINNED) != 0;
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        const size_t off = p->off[(size_t)g], cnt = p->cnt[(size_t)g];
        if (cnt == 0) return FA_OK;
        // after the part's last reducing call: it read the shadow
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.copy, p->done[(size_t)g], 0));
        }
        char* db = p->sign.buf.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * p->sign.stride[(size_t)g];
        ++r.copy_gen;  // the next reducing call waits for the copy stream
        return mx8_h2d(r, db, reinterpret_cast<const char*>(bits + (off >> 5)), sign_words(cnt) * 4, pinned);
    });
    if (rc) return rc;
    return mark_submitted(ctx, *p, slot, 1.0f);
}

// The vote on the current device over n elements: bits[k] at the word of the first one, a multiple of 32 of the bucket.
int sign_on(const fa::Tuning& tu, const uint32_t* const* bits, int D, size_t n, const SignCfg& c, const void* ref,
            fa_dtype rdt, void* dst, fa_dtype odt, uint32_t* neg, uint32_t* pos, hipStream_t s) {
    const fa::SignSplit sp = fa::sign_split(bits, D, n, ref, rdt, dst, odt, neg, pos);
    FA_HIP(fa::launch_sign_vote(bits, D, (int64_t)n, c.eta, c.rule, c.margin, ref, rdt, dst, odt, neg, pos, sp, tu, s));
    return FA_OK;
}

// Before the round's launches: the receipts are there, and the planes' arrays if the round leaves them.
int sign_round_begin(fa_ctx* ctx, Part& p) {
    SignStage& s = p.sign;
    if (!s.buf) return fail(FA_ERR_STATE, "sign: part %d has no sign receipts (fa_submit_sign)", p.id);
    for (size_t g = 0; g < (size_t)ctx->G; ++g)
        if (p.off[g] % 64 || (p.npiece[g] > 1 && p.piece_len[g] % 64))
            return fail(FA_ERR_STATE, "sign: part %d is not cut at multiples of 64 elements", p.id);
    if (!s.cfg.planes || s.planes) return FA_OK;
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, 2 * s.stride[g]); };
    const int g = s.planes.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "sign: plane alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

// Rules 3-9 for piece j of GPU g (the current device), into dst (dtype odt): every client's shadow, the reference in
// the part's output (dst itself where the aggregate is reduced in place).
int sign_piece(fa_ctx* ctx, Part& p, int g, int j, void* dst, fa_dtype odt, hipStream_t st) {
    const SignStage& s = p.sign;
    const size_t lo = piece_lo(p, g, j), cnt = piece_cnt(p, g, j);
    if (cnt == 0) return FA_OK;
    std::vector<const uint32_t*> bits((size_t)p.D);
    for (int k = 0; k < p.D; ++k)
        bits[(size_t)k] = s.buf.at<uint32_t>((size_t)g) + (size_t)k * (s.stride[(size_t)g] / 4) + (lo >> 5);
    const void* ref = s.ref ? static_cast<const char*>(p.dout[(size_t)g]) + lo * dsize(p.out) : nullptr;
    uint32_t* neg = s.cfg.planes ? s.planes.at<uint32_t>((size_t)g) + (lo >> 5) : nullptr;
    return sign_on(ctx->tuning.tu, bits.data(), p.D, cnt, s.cfg, ref, p.out, dst, odt, neg,
                   neg ? neg + s.stride[(size_t)g] / 4 : nullptr, st);
}

// ------------------------------------------------------------------ sparse-sum stage

int check_sparse_clients(int D) {
    if (D < 1 || D > FA_SPARSE_MAX_CLIENTS) return fail(FA_ERR_ARG, "sparse: D = %d clients outside 1 .. %d", D, FA_SPARSE_MAX_CLIENTS);
    return FA_OK;
}

// The shadows and the workspaces of a part, allocated once per k_max: per GPU held x stride bytes, a shadow cap[g] =
// min(k_max, cnt) indices followed by as many values, and one workspace over the GPU's largest piece (its pieces run one
// after the other on one stream).  On failure the part keeps the stage.
int ensure_sparse_buf(fa_ctx* ctx, Part& p) {
    SparseStage& s = p.sparse;
    if (s.buf) return FA_OK;
    s.cap.clear();
    s.stride.clear();
    s.cut.assign((size_t)ctx->G, {});
    for (size_t g = 0; g < (size_t)ctx->G; ++g) {
        s.cap.push_back(std::min(s.cfg.k_max, p.cnt[g]));
        s.stride.push_back((s.cap[g] * 8 + 255) / 256 * 256);
        s.cut[g].assign((size_t)p.D * (size_t)(p.npiece[g] + 1), 0);
    }
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.stride[g]); };
    const auto wbytes = [&](size_t g) {
        size_t most = 0;
        for (int j = 0; j < p.npiece[g]; ++j) most = std::max(most, piece_cnt(p, (int)g, j));
        return std::max<size_t>(256, fa::sparse_workspace(most, p.D));
    };
    int g = s.buf.alloc(ctx->gpu, bytes);
    if (g >= 0) return fail(FA_ERR_NOMEM, "sparse: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
    g = s.work.alloc(ctx->gpu, wbytes);
    if (g < 0) return FA_OK;
    s.buf.free(ctx->gpu);
    return fail(FA_ERR_NOMEM, "sparse: workspace alloc of %zu B failed on GPU %zu", wbytes((size_t)g), (size_t)g);
}

int submit_sparse_impl(fa_ctx* ctx, int part_id, int slot, const uint32_t* idx, const float* val, size_t k, float weight,
                       int flags) {
    Trace tr("fa_submit_sparse part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~FA_HOST_PINNED) return fail(FA_ERR_ARG, "sparse: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    if (!p->sparse.on()) return fail(FA_ERR_STATE, "sparse: part %d has no sparse-sum stage (fa_set_sparse_sum)", part_id);
    if (k > p->sparse.cfg.k_max)
        return fail(FA_ERR_ARG, "sparse: %zu entries, part %d takes at most %zu (fa_set_sparse_sum)", k, part_id, p->sparse.cfg.k_max);
    if (k && (!idx || !val)) return fail(FA_ERR_ARG, "sparse: %s is null", !idx ? "idx" : "val");
    if (k && (uint64_t)p->n > (1ull << 32)) return fail(FA_ERR_ARG, "sparse: part %d holds more than 2^32 elements", part_id);
    if ((uint64_t)k > 0xffffffffull) return fail(FA_ERR_ARG, "sparse: %zu entries, a receipt holds at most 2^32 - 1", k);
    for (size_t j = 0; j < k; ++j) {
        if ((uint64_t)idx[j] >= (uint64_t)p->n) return fail(FA_ERR_ARG, "sparse: idx[%zu] = %u, the bucket holds %zu elements", j, idx[j], p->n);
        if (j && idx[j] <= idx[j - 1])
            return fail(FA_ERR_ARG, "sparse: idx[%zu] = %u after idx[%zu] = %u: not strictly ascending", j, idx[j], j - 1, idx[j - 1]);
    }
    if ((rc = ensure_sparse_buf(ctx, *p))) return rc;
    const bool pinned = (flags & FA_HOST_PINNED) != 0;
    const auto first_at = [&](size_t e) { return (size_t)(std::lower_bound(idx, idx + k, (uint64_t)e, [](uint32_t a, uint64_t b) { return (uint64_t)a < b; }) - idx); };
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        SparseStage& s = p->sparse;
        const size_t off = p->off[(size_t)g], cnt = p->cnt[(size_t)g], np = (size_t)p->npiece[(size_t)g];
        if (cnt == 0) return FA_OK;
        // after the part's last reducing call: it read the shadow
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.copy, p->done[(size_t)g], 0));
        }
        const size_t a = first_at(off), b = first_at(off + cnt);  // the GPU's entries: b - a <= min(k_max, cnt)
        char* di = s.buf.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * s.stride[(size_t)g];
        ++r.copy_gen;  // the next reducing call waits for the copy stream
        int rc2 = mx8_h2d(r, di, reinterpret_cast<const char*>(idx + a), (b - a) * 4, pinned);
        if (!rc2) rc2 = mx8_h2d(r, di + s.cap[(size_t)g] * 4, reinterpret_cast<const char*>(val + a), (b - a) * 4, pinned);
        if (rc2) return rc2;
        uint64_t* cut = &s.cut[(size_t)g][(size_t)slot * (np + 1)];
        for (size_t j = 0; j < np; ++j) cut[j] = first_at(off + piece_lo(*p, g, (int)j)) - a;
        cut[np] = b - a;
        return FA_OK;
    });
    if (rc) return rc;
    return mark_submitted(ctx, *p, slot, weight);
}

// Before the round's launches: the receipts are there (a part's pieces are fixed when it is defined, so the cuts of the
// submits hold).
int sparse_round_begin(const Part& p) {
    if (!p.sparse.buf) return fail(FA_ERR_STATE, "sparse: part %d has no top-k receipts (fa_submit_sparse)", p.id);
    return FA_OK;
}

// Rules 1-2 for piece j of GPU g (the current device), into dst (dtype odt): every client's entries of the piece under
// w, the reference in the part's output (dst itself where the aggregate is reduced in place).
int sparse_piece(fa_ctx* ctx, Part& p, int g, int j, const float* w, void* dst, fa_dtype odt, hipStream_t st) {
    const SparseStage& s = p.sparse;
    const size_t lo = piece_lo(p, g, j), cnt = piece_cnt(p, g, j), np = (size_t)p.npiece[(size_t)g];
    if (cnt == 0) return FA_OK;
    std::vector<const uint32_t*> idx((size_t)p.D);
    std::vector<const float*> val((size_t)p.D);
    std::vector<uint64_t> k((size_t)p.D);
    for (int c = 0; c < p.D; ++c) {
        const char* base = s.buf.at((size_t)g) + (size_t)(c - p.c0[(size_t)g]) * s.stride[(size_t)g];
        const uint64_t a = s.cut[(size_t)g][(size_t)c * (np + 1) + (size_t)j], b = s.cut[(size_t)g][(size_t)c * (np + 1) + (size_t)j + 1];
        idx[(size_t)c] = reinterpret_cast<const uint32_t*>(base) + a;
        val[(size_t)c] = reinterpret_cast<const float*>(base + s.cap[(size_t)g] * 4) + a;
        k[(size_t)c] = b - a;
    }
    const void* ref = s.ref ? static_cast<const char*>(p.dout[(size_t)g]) + lo * dsize(p.out) : nullptr;
    FA_HIP(fa::launch_sparse_sum(idx.data(), val.data(), k.data(), w, p.D, (uint64_t)(p.off[(size_t)g] + lo), (int64_t)cnt, ref,
                                 p.out, dst, odt, s.work.at((size_t)g), -1, ctx->tuning.tu, st));
    return FA_OK;
}

// ------------------------------------------------------------------ MX8-sum stage

int check_mx8sum_clients(int D) {
    if (D < 1 || D > FA_MX8_SUM_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "mx8 sum: D = %d clients outside 1 .. %d", D, FA_MX8_SUM_MAX_CLIENTS);
    return FA_OK;
}

inline size_t mx8_scales(size_t off, size_t cnt);  // below, with the receipts
void mx8_shadow_layout(const Part& p, int G, std::vector<size_t>* stride, std::vector<size_t>* eoff);

// The shadows of a part, allocated once: per GPU held x stride bytes in the MX8 shadow layout.  q lies at the shadow's
// start and a piece starts on a multiple of 64 elements, so every launch takes the vector form.  On failure the part keeps
// the stage.
int ensure_mx8sum_buf(fa_ctx* ctx, Part& p) {
    Mx8SumStage& s = p.mx8sum;
    if (s.buf) return FA_OK;
    mx8_shadow_layout(p, ctx->G, &s.stride, &s.eoff);
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.stride[g]); };
    const int g = s.buf.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "mx8 sum: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

int submit_mx8_sum_impl(fa_ctx* ctx, int part_id, int slot, const int8_t* q, const uint8_t* e, float weight, int flags) {
    Trace tr("fa_submit_mx8_sum part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~FA_HOST_PINNED) return fail(FA_ERR_ARG, "mx8 sum: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    if (!p->mx8sum.on()) return fail(FA_ERR_STATE, "mx8 sum: part %d has no MX8-sum stage (fa_set_mx8_sum)", part_id);
    if (p->n > 0 && (!q || !e)) return fail(FA_ERR_ARG, "mx8 sum: %s is null", !q ? "q" : "e");
    if ((rc = ensure_mx8sum_buf(ctx, *p))) return rc;
    const bool pinned = (flags & FA_HOST_PINNED) != 0;
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        const size_t off = p->off[(size_t)g], cnt = p->cnt[(size_t)g];
        if (cnt == 0) return FA_OK;
        // after the part's last reducing call: it read the shadow
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.copy, p->done[(size_t)g], 0));
        }
        char* dq = p->mx8sum.buf.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * p->mx8sum.stride[(size_t)g];
        ++r.copy_gen;  // the next reducing call waits for the copy stream
        int rc2 = mx8_h2d(r, dq, reinterpret_cast<const char*>(q) + off, cnt, pinned);
        if (!rc2)
            rc2 = mx8_h2d(r, dq + p->mx8sum.eoff[(size_t)g], reinterpret_cast<const char*>(e) + (off >> 5), mx8_scales(off, cnt),
                          pinned);
        return rc2;
    });
    if (rc) return rc;
    return mark_submitted(ctx, *p, slot, weight);
}

// Before the round's launches: the receipts are there.
int mx8sum_round_begin(const Part& p) {
    if (!p.mx8sum.buf) return fail(FA_ERR_STATE, "mx8 sum: part %d has no MX8 receipts (fa_submit_mx8_sum)", p.id);
    return FA_OK;
}

// Rules 1-3 for piece j of GPU g (the current device), into dst (dtype odt): every client's codes and scales of the piece
// under w, the reference in the part's output (dst itself where the aggregate is reduced in place).
int mx8sum_piece(fa_ctx* ctx, Part& p, int g, int j, const float* w, void* dst, fa_dtype odt, hipStream_t st) {
    const Mx8SumStage& s = p.mx8sum;
    const size_t off = p.off[(size_t)g], lo = piece_lo(p, g, j), cnt = piece_cnt(p, g, j);
    if (cnt == 0) return FA_OK;
    std::vector<const int8_t*> q((size_t)p.D);
    std::vector<const uint8_t*> e((size_t)p.D);
    for (int c = 0; c < p.D; ++c) {
        const char* base = s.buf.at((size_t)g) + (size_t)(c - p.c0[(size_t)g]) * s.stride[(size_t)g];
        q[(size_t)c] = reinterpret_cast<const int8_t*>(base) + lo;
        e[(size_t)c] = reinterpret_cast<const uint8_t*>(base) + s.eoff[(size_t)g] + (((off + lo) >> 5) - (off >> 5));
    }
    const void* ref = s.ref ? static_cast<const char*>(p.dout[(size_t)g]) + lo * dsize(p.out) : nullptr;
    FA_HIP(fa::launch_mx8_sum(q.data(), e.data(), w, p.D, (uint64_t)(off + lo), (int64_t)cnt, ref, p.out, dst, odt,
                              ctx->tuning.tu, st));
    return FA_OK;
}

// ------------------------------------------------------------------ low-rank-sum stage

int check_lrsum_clients(int D) {
    if (D < 1 || D > FA_LOWRANK_SUM_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "lowrank sum: D = %d clients outside 1 .. %d", D, FA_LOWRANK_SUM_MAX_CLIENTS);
    return FA_OK;
}

// The factor shadows of a part, allocated once per table and r_max: per GPU held x fstride bytes, a shadow the whole
// receipt at rank r_max.  On failure the part keeps the stage.
int ensure_lrsum_buf(fa_ctx* ctx, Part& p) {
    LowrankSumStage& s = p.lrsum;
    if (s.factors) return FA_OK;
    s.fstride = ((size_t)fa::lowrank_len(s.cfg.mats.data(), s.cfg.mats.size(), p.n, s.cfg.r_max) * 4 + 255) / 256 * 256;
    s.rank.assign((size_t)p.D, 0);
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.fstride); };
    const int g = s.factors.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "lowrank sum: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

int submit_lowrank_sum_impl(fa_ctx* ctx, int part_id, int slot, const float* f, size_t len, int r, float weight, int flags) {
    Trace tr("fa_submit_lowrank_sum part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~FA_HOST_PINNED) return fail(FA_ERR_ARG, "lowrank sum: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    const LowrankSumCfg& c = p->lrsum.cfg;
    if (!c.on()) return fail(FA_ERR_STATE, "lowrank sum: part %d has no low-rank-sum stage (fa_set_lowrank_sum)", part_id);
    if (r < 1 || r > c.r_max)
        return fail(FA_ERR_ARG, "lowrank sum: rank %d, part %d takes 1 .. %d (fa_set_lowrank_sum)", r, part_id, c.r_max);
    const size_t need = (size_t)fa::lowrank_len(c.mats.data(), c.mats.size(), p->n, r);
    if (len != need)
        return fail(FA_ERR_ARG, "lowrank sum: %zu values, a receipt of rank %d for part %d has %zu (fa_lowrank_len)", len, r, part_id, need);
    if (len && !f) return fail(FA_ERR_ARG, "lowrank sum: f is null");
    if ((rc = ensure_lrsum_buf(ctx, *p))) return rc;
    const bool pinned = (flags & FA_HOST_PINNED) != 0;
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& gr = ctx->gpu[(size_t)g];
        DeviceGuard dg(gr.dev);
        if (p->cnt[(size_t)g] == 0) return FA_OK;
        // after the part's last reducing call: it read the shadow
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(gr.copy, p->done[(size_t)g], 0));
        }
        char* df = p->lrsum.factors.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * p->lrsum.fstride;
        ++gr.copy_gen;  // the next reducing call waits for the copy stream
        return mx8_h2d(gr, df, reinterpret_cast<const char*>(f), len * 4, pinned);
    });
    if (rc) return rc;
    p->lrsum.rank[(size_t)slot] = r;
    return mark_submitted(ctx, *p, slot, weight);
}

// Before the round's launches: the receipts are there.
int lowranksum_round_begin(const Part& p) {
    if (!p.lrsum.factors) return fail(FA_ERR_STATE, "lowrank sum: part %d has no low-rank receipts (fa_submit_lowrank_sum)", p.id);
    return FA_OK;
}

// Rules 1-4 for piece j of GPU g (the current device), into dst (dtype odt): every client's whole receipt under w with
// the piece's plan, the reference in the part's output (dst itself where the aggregate is reduced in place).
int lowranksum_piece(fa_ctx* ctx, Part& p, int g, int j, const float* w, void* dst, fa_dtype odt, hipStream_t st) {
    const LowrankSumStage& s = p.lrsum;
    const size_t lo = piece_lo(p, g, j), cnt = piece_cnt(p, g, j);
    if (cnt == 0) return FA_OK;
    std::vector<const float*> f((size_t)p.D);
    for (int c = 0; c < p.D; ++c)
        f[(size_t)c] = reinterpret_cast<const float*>(s.factors.at((size_t)g) + (size_t)(c - p.c0[(size_t)g]) * s.fstride);
    const void* ref = s.ref ? static_cast<const char*>(p.dout[(size_t)g]) + lo * dsize(p.out) : nullptr;
    FA_HIP(fa::launch_lowrank_sum(s.plan.at((size_t)g) + s.plan_at[(size_t)g][(size_t)j], s.plan_len[(size_t)g][(size_t)j], f.data(),
                                  s.rank.data(), w, p.D, (uint64_t)(p.off[(size_t)g] + lo), (int64_t)cnt, ref, p.out, dst, odt, st));
    return FA_OK;
}

// ------------------------------------------------------------------ rot1-sum stage

int check_rot1sum_clients(int D) {
    if (D < 1 || D > FA_ROT1_SUM_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "rot1 sum: D = %d clients outside 1 .. %d", D, FA_ROT1_SUM_MAX_CLIENTS);
    return FA_OK;
}

inline size_t rot1_blocks(size_t off, size_t cnt);  // below, with the receipts
void rot1_shadow_layout(const Part& p, int G, std::vector<size_t>* stride, std::vector<size_t>* soff);

// The shadows of a part, allocated once: per GPU held x stride bytes in the rot1 shadow layout.  On failure the part
// keeps the stage.
int ensure_rot1sum_buf(fa_ctx* ctx, Part& p) {
    Rot1SumStage& s = p.rot1sum;
    if (s.buf) return FA_OK;
    rot1_shadow_layout(p, ctx->G, &s.stride, &s.soff);
    s.seed.assign((size_t)p.D, 0);
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.stride[g]); };
    const int g = s.buf.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "rot1 sum: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

int submit_rot1_sum_impl(fa_ctx* ctx, int part_id, int slot, const uint32_t* bits, const float* scale, uint64_t seed,
                         float weight, int flags) {
    Trace tr("fa_submit_rot1_sum part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~FA_HOST_PINNED) return fail(FA_ERR_ARG, "rot1 sum: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    if (!p->rot1sum.on()) return fail(FA_ERR_STATE, "rot1 sum: part %d has no rot1-sum stage (fa_set_rot1_sum)", part_id);
    if (p->n > 0 && (!bits || !scale)) return fail(FA_ERR_ARG, "rot1 sum: %s is null", !bits ? "bits" : "scale");
    if ((rc = ensure_rot1sum_buf(ctx, *p))) return rc;
    const bool pinned = (flags & FA_HOST_PINNED) != 0;
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        const size_t off = p->off[(size_t)g], cnt = p->cnt[(size_t)g];
        if (cnt == 0) return FA_OK;
        // after the part's last reducing call: it read the shadow
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.copy, p->done[(size_t)g], 0));
        }
        const size_t b0 = off >> 12, nb = rot1_blocks(off, cnt);
        char* db = p->rot1sum.buf.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * p->rot1sum.stride[(size_t)g];
        ++r.copy_gen;  // the next reducing call waits for the copy stream
        int rc2 = mx8_h2d(r, db, reinterpret_cast<const char*>(bits + b0 * fa::kRot1Words), nb * fa::kRot1Words * 4, pinned);
        if (!rc2) rc2 = mx8_h2d(r, db + p->rot1sum.soff[(size_t)g], reinterpret_cast<const char*>(scale + b0), nb * 4, pinned);
        return rc2;
    });
    if (rc) return rc;
    p->rot1sum.seed[(size_t)slot] = seed;
    return mark_submitted(ctx, *p, slot, weight);
}

// Before the round's launches: the receipts are there.
int rot1sum_round_begin(const Part& p) {
    if (!p.rot1sum.buf) return fail(FA_ERR_STATE, "rot1 sum: part %d has no rot1 receipts (fa_submit_rot1_sum)", p.id);
    return FA_OK;
}

// Rules 0-6 for piece j of GPU g (the current device), into dst (dtype odt): every client's words and scales from the
// piece's first block on under w, the reference in the part's output (dst itself where the aggregate is reduced in place).
int rot1sum_piece(fa_ctx* ctx, Part& p, int g, int j, const float* w, void* dst, fa_dtype odt, hipStream_t st) {
    const Rot1SumStage& s = p.rot1sum;
    const size_t off = p.off[(size_t)g], lo = piece_lo(p, g, j), cnt = piece_cnt(p, g, j);
    if (cnt == 0) return FA_OK;
    const size_t pb = ((off + lo) >> 12) - (off >> 12);  // the piece's first block among the GPU's
    std::vector<const uint32_t*> bits((size_t)p.D);
    std::vector<const float*> scale((size_t)p.D);
    for (int c = 0; c < p.D; ++c) {
        const char* base = s.buf.at((size_t)g) + (size_t)(c - p.c0[(size_t)g]) * s.stride[(size_t)g];
        bits[(size_t)c] = reinterpret_cast<const uint32_t*>(base) + pb * fa::kRot1Words;
        scale[(size_t)c] = reinterpret_cast<const float*>(base + s.soff[(size_t)g]) + pb;
    }
    const void* ref = s.ref ? static_cast<const char*>(p.dout[(size_t)g]) + lo * dsize(p.out) : nullptr;
    FA_HIP(fa::launch_rot1_sum(bits.data(), scale.data(), s.seed.data(), w, p.D, (uint64_t)(off + lo), (int64_t)cnt, ref, p.out,
                               dst, odt, ctx->tuning.tu, st));
    return FA_OK;
}

// ------------------------------------------------------------------ one reducing call, as the stages see it

int stage_round_begin(fa_ctx* ctx, Part& p, const float* w, hipStream_t s, StageRound* rd) {
    if (p.noise.on() && p.noise.round >= kNoiseRounds)
        return fail(FA_ERR_STATE, "noise: part %d has used all 2^32 rounds of its seed (fa_set_noise a new seed and "
                                  "fa_noise_set_round)", p.id);
    // a clip stage with a reference: the norm pass and the host's wait for its sums (without a reference the round is
    // the bootstrap: the plain aggregate, reported as unclipped)
    if (ClipStage& c = p.clip; c.on()) {
        c.q.assign((size_t)p.D, 0.0);
        c.s.assign((size_t)p.D, 1.0f);
        c.in.assign((size_t)p.D, 1);
        c.n = 0;
        c.reported = true;
        rd->subset = c.has_ref;
        if (c.has_ref)
            if (int rc = clip_plan(ctx, p, w, s, &rd->plan)) return rc;
    }
    // Krum, geomed, DnC (never with each other or with clip) and Bulyan (an FA_TRIMMED part: never with those three): the
    // passes, the host's waits for their results, and the selection or the new weights
    if (p.krum.on() || p.geomed.on() || p.dnc.on()) rd->subset = true;
    if (p.krum.on()) return krum_plan(ctx, p, w, s, &rd->plan);
    if (p.dnc.on()) return dnc_plan(ctx, p, w, s, &rd->plan);
    if (p.geomed.on()) return geomed_plan(ctx, p, w, s, &rd->plan);
    if (p.bulyan.on()) return bulyan_plan(ctx, p, s, &rd->plan);
    if (p.secagg.on()) return secagg_round_begin(ctx, p, s);
    if (p.sign.on()) return sign_round_begin(ctx, p);
    if (p.sparse.on()) return sparse_round_begin(p);
    if (p.mx8sum.on()) return mx8sum_round_begin(p);
    if (p.lrsum.on()) return lowranksum_round_begin(p);
    if (p.rot1sum.on()) return rot1sum_round_begin(p);
    return FA_OK;
}

// The aggregate (the plain chain, a plan's chain, Bulyan's centred mean or the unmasked sum of a secagg part)
// into adst (dst without a server optimizer or a noise stage; with one in fp32 -- an f32 part: in its
// output, where the stages then run in place), then the noise (in place before a server optimizer, else into dst with the
// one rounding), then one step or the bootstrap of a part without a master, then the new clip reference.
int stage_piece(fa_ctx* ctx, Part& p, int g, int j, const float* w, const StageRound& rd, std::vector<const void*>& ptrs,
                hipStream_t st) {
    const fa::Tuning& tu = ctx->tuning.tu;
    const size_t lo = piece_lo(p, g, j), cnt = piece_cnt(p, g, j);
    void* dst = static_cast<char*>(p.dout[(size_t)g]) + lo * dsize(p.out);
    const bool opt = p.opt.on(), noisy = p.noise.on(), wide = opt || noisy;
    float* avg = !wide ? nullptr : p.out == FA_F32 ? static_cast<float*>(dst) : p.oavg.at<float>((size_t)g) + lo;
    void* adst = wide ? (void*)avg : dst;
    const fa_dtype adt = wide ? FA_F32 : p.out;
    int rc;
    if (rd.subset)
        rc = subset_chain(ctx, p, g, j, rd.plan, adst, adt, st);
    else if (p.bulyan.on())
        rc = bulyan_piece(ctx, p, g, j, rd.plan, adst, adt, st);
    else if (p.secagg.on())
        rc = secagg_piece(ctx, p, g, j, ptrs, adst, adt, st);
    else if (p.sign.on())
        rc = sign_piece(ctx, p, g, j, adst, adt, st);
    else if (p.sparse.on())
        rc = sparse_piece(ctx, p, g, j, w, adst, adt, st);
    else if (p.mx8sum.on())
        rc = mx8sum_piece(ctx, p, g, j, w, adst, adt, st);
    else if (p.lrsum.on())
        rc = lowranksum_piece(ctx, p, g, j, w, adst, adt, st);
    else if (p.rot1sum.on())
        rc = rot1sum_piece(ctx, p, g, j, w, adst, adt, st);
    else
        rc = reduce_on(ctx, g, tu, piece_ptrs(p, g, j, 0, p.D, ptrs), w, p.D, cnt, p.in, adst, adt, p.mode,
                       mode_arg(p.mode, p.divisor, p.trim, p.D), nullptr, st);
    if (!rc && noisy)
        rc = noise_on(tu, avg, opt ? (void*)avg : dst, opt ? FA_F32 : p.out, p.noise.cfg.stddev, p.noise.cfg.seed,
                      (uint32_t)p.id, (uint32_t)p.noise.round, (uint64_t)(p.off[(size_t)g] + lo), cnt, st);
    if (!rc && opt)
        rc = opt_on(tu, p.opt.master ? p.opt.cfg.rule : fa::kOptBoot, p.opt.cfg, avg, p.opt.x.at<float>((size_t)g) + lo,
                    p.opt.m.at<float>((size_t)g) + lo, opt_adaptive(p.opt.cfg.rule) ? p.opt.v.at<float>((size_t)g) + lo : nullptr,
                    cnt, dst, p.out, st);
    // with a reply stage the output is not final yet: the reference is taken after it (stage_gpu_end)
    if (!rc && p.clip.on() && !p.reply.on()) rc = clip_take_reference(p, g, j, st);
    return rc;
}

int stage_gpu_end(fa_ctx* ctx, Part& p, int g, hipStream_t st) {
    if (!p.reply.on()) return FA_OK;  // y -> g' over the GPU's whole range, then the clip stage's reference from g'
    int rc = reply_stage(ctx, p, g, st);
    for (int j = 0; !rc && p.clip.on() && j < p.npiece[(size_t)g]; ++j) rc = clip_take_reference(p, g, j, st);
    return rc;
}

void stage_round_end(Part& p) {
    if (p.reply.on()) reply_round_done(p);
    if (p.opt.on()) {  // one reducing call = one step (the first one without a master: none)
        if (p.opt.master) ++p.opt.steps;
        p.opt.master = true;
    }
    if (p.clip.on()) p.clip.has_ref = true;  // what this round sent out
    if (p.noise.on()) ++p.noise.round;       // one reducing call = one round of the generator
    if (p.secagg.on()) p.secagg.have = false;  // terms are per round: a stale list is never applied
    if (p.sign.on()) p.sign.has_planes = p.sign.cfg.planes;
}

// ------------------------------------------------------------------ setting a stage on a part

// Waits for the devices of the context: for everything that may touch a part's stage state.  A reduction may have run
// on a caller's stream that is gone by now, so this waits for the devices, not for a stream handle (state reads,
// writes, rule changes and removals are rare).
int wait_devices(fa_ctx* ctx) {
    for (int g = 0; g < ctx->G; ++g) {
        DeviceGuard dg(ctx->gpu[(size_t)g].dev);
        FA_HIP(hipDeviceSynchronize());
    }
    return FA_OK;
}

// fa_set_server_opt on a part (o checked; not FA_LITERAL, not rs).  None: the stage and its state go.  The
// same rule: only the hyperparameters change.  Another rule (or the first one): the arrays the rule needs are
// allocated, x is kept when the part had a stage, m and v are zeroed.
int set_part_opt(fa_ctx* ctx, Part& p, const OptCfg& o) {
    OptStage& s = p.opt;
    if (!o.on()) {
        free_opt(ctx, p);
        return FA_OK;
    }
    if (o.rule == s.cfg.rule) {
        s.cfg = o;
        return FA_OK;
    }
    const bool fresh = !s.on(), with_v = opt_adaptive(o.rule);
    if (!fresh)  // the arrays about to be zeroed or freed may still be in use
        if (int rc = wait_devices(ctx)) return rc;
    if (!with_v) s.v.free(ctx->gpu);
    int rc = FA_OK;
    for (DevArrays* a : {&s.x, &s.m, &s.v}) {
        if (*a || (a == &s.v && !with_v)) continue;
        const int g = a->alloc(ctx->gpu, [&](size_t i) { return f32_bytes(p, i); });
        if (g >= 0)
            rc = fail(FA_ERR_NOMEM, "server opt: state alloc of %zu B failed on GPU %zu", f32_bytes(p, (size_t)g), (size_t)g);
        if (rc) break;
    }
    const auto zero = [&]() -> int {  // x of a part that had no stage, m, v
        for (size_t g = 0; g < (size_t)ctx->G; ++g) {
            DeviceGuard dg(ctx->gpu[g].dev);
            for (DevArrays* a : {&s.x, &s.m, &s.v})
                if (*a && (a != &s.x || fresh)) FA_HIP(hipMemset(a->at(g), 0, f32_bytes(p, g)));
        }
        return wait_devices(ctx);  // the null stream's zeroing: the context's non-blocking streams do not wait for it
    };
    if (!rc) rc = zero();
    if (!rc) {
        s.cfg = o;
        rc = ensure_oavg(ctx, p, "server opt");
    }
    if (rc) {
        free_opt(ctx, p);
        return rc;
    }
    // A rule change leaves a round already stepped as it is: the finalize after it copies out, one step per round.
    if (fresh) restart_round_plain(p);
    return FA_OK;
}

// fa_set_clip on a part (max_norm checked; an FA_FEDAVG part, not rs).  0: the stage and its arrays go.  A part
// that has the stage: only the bound changes.  Else the reference (and a 16-bit part's first-term buffer) is
// allocated; the part has no reference until a round or fa_clip_set_reference gives it one.
int set_part_clip(fa_ctx* ctx, Part& p, const ClipCfg& c) {
    ClipStage& s = p.clip;
    if (!c.on()) {
        if (s.on())  // the arrays may still be in use
            if (int rc = wait_devices(ctx)) return rc;
        free_clip(ctx, p);
        return FA_OK;
    }
    if (!s.on()) {
        const auto bytes = [&](size_t i) { return f32_bytes(p, i); };
        int g = s.ref.alloc(ctx->gpu, bytes);
        if (g < 0 && p.in != FA_F32) g = s.init.alloc(ctx->gpu, bytes);
        if (g >= 0) {
            free_clip(ctx, p);
            return fail(FA_ERR_NOMEM, "clip: reference alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
        }
        restart_round_plain(p);
    }
    s.cfg = c;
    return FA_OK;
}

// fa_set_krum / fa_set_geomed on a part (the stage's numbers checked against D; an FA_FEDAVG part, not rs).  Off: the
// stage and its report go.  Else the numbers change; a part that had no such stage starts without a report.
template <class Stage, class Cfg>
int set_part_select(Part& p, Stage& s, const Cfg& c) {
    if (!c.on()) {
        s = Stage{};
        return FA_OK;
    }
    if (!s.on()) {
        s.reported = false;
        restart_round_plain(p);
    }
    s.cfg = c;
    return FA_OK;
}

// fa_set_bulyan on a part (f checked against D; an FA_TRIMMED part, not rs).
int set_part_bulyan(Part& p, const BulyanCfg& c) {
    if (p.bulyan.on() || c.on()) p.ready = false;
    if (!p.bulyan.on() || !c.on()) p.bulyan = BulyanStage{};  // the stage and its report go, or it starts without one
    p.bulyan.cfg = c;
    return FA_OK;
}

// fa_set_noise on a part (stddev checked; not FA_LITERAL, not rs).  0: the stage goes, and the aggregate buffer
// unless a server optimizer keeps it.  A part that has the stage: stddev and seed change, the round stays.
// Else the stage starts at round 0, a 16-bit part gets its fp32 aggregate buffer.
int set_part_noise(fa_ctx* ctx, Part& p, const NoiseCfg& c) {
    const bool fresh = !p.noise.on();
    if (fresh || !c.on()) p.noise = NoiseStage{};
    int rc = FA_OK;
    if (c.on()) {
        p.noise.cfg.stddev = c.stddev;
        rc = ensure_oavg(ctx, p, "noise");
        if (rc && fresh) p.noise = NoiseStage{};
    }
    drop_oavg_if_unused(ctx, p);
    if (rc || !c.on()) return rc;
    p.noise.cfg.seed = c.seed;
    if (fresh) restart_round_plain(p);
    return FA_OK;
}

// fa_set_mx8 / fa_set_topk / fa_set_lowrank / fa_set_rot1 / fa_set_mx8_reply on a part (not FA_LITERAL, not rs).  Off: what the stage
// allocated goes, after the devices' pending work.  On, for a part without it: what this round kept host-side or chained
// so far goes back to the plain path; the buffers come with the first fa_submit_mx8 / fa_submit_topk /
// fa_submit_lowrank, or the first reducing call.
int set_part_flag(fa_ctx* ctx, Part& p, bool reply, bool on) {
    const bool was = reply ? p.reply.on() : p.mx8.on();
    if (on == was) return FA_OK;
    if (int rc = on ? host_flush(ctx, p) : wait_devices(ctx)) return rc;
    if (!on) {
        reply ? free_reply(ctx, p) : free_mx8(ctx, p);
        return FA_OK;
    }
    restart_round_plain(p);
    (reply ? p.reply.cfg.flag : p.mx8.cfg.flag) = true;
    return FA_OK;
}

// The low-rank plans of a part over the table m (the receipt format's, or the low-rank-sum stage's): per GPU one
// allocation with the plan of every piece's range, uploaded with a plain copy (a setter is no hot path).
int upload_plans(fa_ctx* ctx, Part& p, const std::vector<fa_lowrank_mat>& m, DevArrays& plan,
                 std::vector<std::vector<size_t>>& plan_at, std::vector<std::vector<size_t>>& plan_len) {
    std::vector<std::vector<char>> blob((size_t)ctx->G);
    plan_at.assign((size_t)ctx->G, {});
    plan_len.assign((size_t)ctx->G, {});
    for (int g = 0; g < ctx->G; ++g)
        for (int j = 0; j < p.npiece[(size_t)g] && p.cnt[(size_t)g]; ++j) {
            const uint64_t i0 = p.off[(size_t)g] + piece_lo(p, g, j), pc = piece_cnt(p, g, j);
            const size_t at = blob[(size_t)g].size(), len = fa::lowrank_plan_bytes(m.data(), m.size(), p.n, i0, pc);
            blob[(size_t)g].resize(at + len);
            fa::lowrank_plan_build(m.data(), m.size(), p.n, i0, pc, blob[(size_t)g].data() + at);
            plan_at[(size_t)g].push_back(at);
            plan_len[(size_t)g].push_back(len);
        }
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, blob[g].size()); };
    const int bad = plan.alloc(ctx->gpu, bytes);
    if (bad >= 0) return fail(FA_ERR_NOMEM, "lowrank: plan alloc of %zu B failed on GPU %d", bytes((size_t)bad), bad);
    for (size_t g = 0; g < (size_t)ctx->G; ++g) {
        DeviceGuard dg(ctx->gpu[g].dev);
        if (!blob[g].empty()) FA_HIP(hipMemcpy(plan.at(g), blob[g].data(), blob[g].size(), hipMemcpyHostToDevice));
    }
    return FA_OK;
}
int upload_lowrank_plans(fa_ctx* ctx, Part& p) {
    return upload_plans(ctx, p, p.mx8.cfg.mats, p.mx8.plan, p.mx8.plan_at, p.mx8.plan_len);
}

// The receipt stage of a part becomes c (any of MX8, top-k and low-rank, or none).  The stage itself goes on and off as
// above; while it stays on, a format that leaves, a k_max that changes, and a table or r_max that changes free that
// format's shadows alone.  A new table's plans are uploaded before the config takes it.
int set_part_receipts(fa_ctx* ctx, Part& p, const ReceiptCfg& c) {
    const ReceiptCfg was = p.mx8.cfg;
    const bool new_lr = !c.same_lowrank(was);
    if (!c.on() || !was.on()) {
        if (int rc = set_part_flag(ctx, p, false, c.on())) return rc;
        if (!c.on()) return FA_OK;
        p.mx8.cfg = c;
    } else {
        const bool drop_q = was.flag && !c.flag && p.mx8.buf, drop_s = was.k_max != c.k_max && p.mx8.sparse;
        const bool drop_f = new_lr && (p.mx8.plan || p.mx8.factors), drop_r = was.rot1 && !c.rot1 && p.mx8.rot;
        if (drop_q || drop_s || drop_f || drop_r)
            if (int rc = wait_devices(ctx)) return rc;
        if (drop_q) p.mx8.buf.free(ctx->gpu);
        if (drop_r) p.mx8.rot.free(ctx->gpu);
        if (drop_s) p.mx8.sparse.free(ctx->gpu);
        if (drop_f) {
            p.mx8.plan.free(ctx->gpu);
            p.mx8.factors.free(ctx->gpu);
        }
        p.mx8.cfg = c;
    }
    if (new_lr && c.lowrank())
        if (int rc = upload_lowrank_plans(ctx, p)) {  // the part keeps the stage without the format
            p.mx8.cfg.mats.clear();
            p.mx8.cfg.r_max = 0;
            if (!p.mx8.cfg.on()) free_mx8(ctx, p);
            return rc;
        }
    return FA_OK;
}

// fa_set_secagg on a part (scale checked; an FA_FEDAVG part with f32 slots, not rs).  Off: the table and the terms go,
// after the devices' pending work.  A part that has the stage: only the scale changes.  Else the round so far goes
// back to the plain path; the round has no terms until fa_secagg_set_terms.
int set_part_secagg(fa_ctx* ctx, Part& p, const SecaggCfg& c) {
    if (!c.on()) {
        if (p.secagg.on())
            if (int rc = wait_devices(ctx)) return rc;
        free_secagg(ctx, p);
        return FA_OK;
    }
    if (!p.secagg.on()) {
        if (int rc = host_flush(ctx, p)) return rc;
        restart_round_plain(p);
    }
    p.secagg.cfg = c;
    return FA_OK;
}

// fa_set_sign on a part (the numbers checked; an FA_FEDAVG part, not rs).  Off: the shadows and the planes go, after the
// devices' pending work.  A part that has the stage: the numbers change; planes that are no longer asked for go.  Else
// what the round received so far is dropped: dense receipts are no sign receipts.
int set_part_sign(fa_ctx* ctx, Part& p, const SignCfg& c) {
    if (c.on() && c.planes && (p.opt.on() || p.noise.on()))
        return fail(FA_ERR_STATE, "sign: part %d has a %s stage: its reply is no function of the vote planes", p.id,
                    p.opt.on() ? "server-optimizer" : "noise");
    if (!c.on() || (p.sign.on() && p.sign.cfg.planes && !c.planes)) {
        if (p.sign.on())
            if (int rc = wait_devices(ctx)) return rc;
        if (!c.on()) {
            free_sign(ctx, p);
            return FA_OK;
        }
        p.sign.planes.free(ctx->gpu);
        p.sign.has_planes = false;
    }
    if (!p.sign.on()) {
        if (int rc = host_flush(ctx, p)) return rc;
        reset_round(p);
    }
    p.sign.cfg = c;
    return FA_OK;
}

// fa_set_sparse_sum on a part (an FA_FEDAVG part of at most FA_SPARSE_MAX_CLIENTS clients, not rs).  Off: the shadows and
// the workspaces go, after the devices' pending work.  Another k_max: they go as well and come anew with the next receipt,
// and with them what the round received; the reference stays (the part's output, rule 4).  The first time: what the round received so far is dropped: dense receipts are
// no top-k receipts.
int set_part_sparse(fa_ctx* ctx, Part& p, const SparseCfg& c) {
    if (p.sparse.on() && c.k_max == p.sparse.cfg.k_max) return FA_OK;
    if (p.sparse.on()) {
        if (int rc = wait_devices(ctx)) return rc;
        const bool held = (bool)p.sparse.buf, ref = p.sparse.ref;
        free_sparse(ctx, p);
        if (!c.on()) return FA_OK;
        p.sparse.ref = ref;  // the stage stays on: the part's output is still its reference (rule 4)
        if (held) reset_round(p);
    } else {
        if (!c.on()) return FA_OK;
        if (int rc = host_flush(ctx, p)) return rc;
        reset_round(p);
    }
    p.sparse.cfg = c;
    return FA_OK;
}

// fa_set_mx8_sum on a part (an FA_FEDAVG part of at most FA_MX8_SUM_MAX_CLIENTS clients, not rs).  Off: the shadows go,
// after the devices' pending work.  On a part that has the stage: nothing.  The first time: what the round received so
// far is dropped: dense receipts are no MX8 receipts.
int set_part_mx8sum(fa_ctx* ctx, Part& p, const Mx8SumCfg& c) {
    if (p.mx8sum.on() == c.on()) return FA_OK;
    if (!c.on()) {
        if (int rc = wait_devices(ctx)) return rc;
        free_mx8sum(ctx, p);
        return FA_OK;
    }
    if (int rc = host_flush(ctx, p)) return rc;
    reset_round(p);
    p.mx8sum.cfg = c;
    return FA_OK;
}

// fa_set_lowrank_sum on a part (an FA_FEDAVG part of at most FA_LOWRANK_SUM_MAX_CLIENTS clients, not rs).  Off: the plans
// and the shadows go, after the devices' pending work.  The same table and r_max: nothing.  Another: they go as well and
// with them what the round received; the reference stays (the part's output).  The first time: what the round received
// so far is dropped: dense receipts are no low-rank receipts.  The plans are uploaded before the config takes the table.
int set_part_lrsum(fa_ctx* ctx, Part& p, const LowrankSumCfg& c) {
    if (p.lrsum.on() && c.same(p.lrsum.cfg)) return FA_OK;
    bool ref = false;
    if (p.lrsum.on()) {
        if (int rc = wait_devices(ctx)) return rc;
        ref = p.lrsum.ref;
        free_lrsum(ctx, p);
        if (!c.on()) return FA_OK;
    } else {
        if (!c.on()) return FA_OK;
        if (int rc = host_flush(ctx, p)) return rc;
    }
    reset_round(p);
    if (int rc = upload_plans(ctx, p, c.mats, p.lrsum.plan, p.lrsum.plan_at, p.lrsum.plan_len)) {
        free_lrsum(ctx, p);
        return rc;
    }
    p.lrsum.cfg = c;
    p.lrsum.ref = ref;
    return FA_OK;
}

// fa_set_rot1_sum on a part (an FA_FEDAVG part of at most FA_ROT1_SUM_MAX_CLIENTS clients, not rs).  Off: the shadows go,
// after the devices' pending work.  On a part that has the stage: nothing.  The first time: what the round received so
// far is dropped: dense receipts are no rot1 receipts.
int set_part_rot1sum(fa_ctx* ctx, Part& p, const Rot1SumCfg& c) {
    if (p.rot1sum.on() == c.on()) return FA_OK;
    if (!c.on()) {
        if (int rc = wait_devices(ctx)) return rc;
        free_rot1sum(ctx, p);
        return FA_OK;
    }
    if (int rc = host_flush(ctx, p)) return rc;
    reset_round(p);
    p.rot1sum.cfg = c;
    return FA_OK;
}

int set_part_stage(fa_ctx* ctx, Part& p, StageId id, const StageCfgs& c) {
    switch (id) {
        case kRot1Sum: return set_part_rot1sum(ctx, p, c.rot1sum);
        case kLowrankSum: return set_part_lrsum(ctx, p, c.lrsum);
        case kMx8Sum: return set_part_mx8sum(ctx, p, c.mx8sum);
        case kSparse: return set_part_sparse(ctx, p, c.sparse);
        case kSign: return set_part_sign(ctx, p, c.sign);
        case kOpt: return set_part_opt(ctx, p, c.opt);
        case kClip: return set_part_clip(ctx, p, c.clip);
        case kKrum: return set_part_select(p, p.krum, c.krum);
        case kGeomed: return set_part_select(p, p.geomed, c.geomed);
        case kBulyan: return set_part_bulyan(p, c.bulyan);
        case kNoise: return set_part_noise(ctx, p, c.noise);
        case kSecagg: return set_part_secagg(ctx, p, c.secagg);
        case kDnc: return set_part_select(p, p.dnc, c.dnc);
        case kMx8: return set_part_receipts(ctx, p, c.mx8);
        default: return set_part_flag(ctx, p, true, c.reply.flag);
    }
}

// ------------------------------------------------------------------ the admission rule

// One row per stage, in StageId order: its name as the refusals begin, its name as in "has a Krum stage", the bucket
// modes it applies to (a bit per fa_mode), whether it belongs to the measure-then-select family (at most one per part,
// and at most one among the context defaults), the stages outside the family it never shares a part with, and the
// tails of its refusals of an rs context and of a part's mode.
struct StageRule {
    const char *name, *title;
    unsigned modes;
    bool family;
    unsigned never;
    const char *rs_tail, *mode_tail;
};
constexpr unsigned kAvg = 1u << FA_FEDAVG, kTrim = 1u << FA_TRIMMED;
const StageRule kRules[kStages] = {
    {"server opt", "server-optimizer", kAvg | kTrim, false, 0, "its aggregate is not bit-specified", ""},
    {"clip", "clip", kAvg, true, 0, "its aggregate is not bit-specified; use FA_SHARD_RANGE", " (the stage clips FA_FEDAVG updates)"},
    {"krum", "Krum", kAvg, true, 0, "a pair's distance needs both clients on one GPU; use FA_SHARD_RANGE",
     " (the stage selects the owners of an FA_FEDAVG average)"},
    {"geomed", "geomed", kAvg, true, 0, "a distance needs every client of an element on one GPU; use FA_SHARD_RANGE",
     " (the stage re-weights the owners of an FA_FEDAVG average)"},
    {"bulyan", "Bulyan", kTrim, false, 0, "the rule needs every client on one GPU; use FA_SHARD_RANGE",
     " (the stage replaces the window of an FA_TRIMMED part)"},
    {"noise", "noise", kAvg | kTrim, false, 0, "its aggregate is not bit-specified; use FA_SHARD_RANGE", ""},
    {"mx8", "MX8", kAvg | kTrim, false, 1u << kSecagg | 1u << kSign | 1u << kSparse | 1u << kMx8Sum | 1u << kLowrankSum | 1u << kRot1Sum, "a GPU holding a whole slot does not hold the matching output; use FA_SHARD_RANGE", ""},
    {"mx8 reply", "reply", kAvg | kTrim, false, 0, "use FA_SHARD_RANGE", ""},
    {"secagg", "secagg", kAvg, true, 1u << kMx8, "its sum is taken over every client of an element; use FA_SHARD_RANGE",
     " (the stage unmasks the sum of an FA_FEDAVG part)"},
    {"dnc", "DnC", kAvg, true, 0, "a Gram entry needs both clients on one GPU; use FA_SHARD_RANGE",
     " (the stage selects the owners of an FA_FEDAVG average)"},
    {"sign", "sign-vote", kAvg, true, 1u << kMx8, "its counts are taken over every client of an element; use FA_SHARD_RANGE",
     " (the stage votes on the updates of an FA_FEDAVG part)"},
    {"sparse", "sparse-sum", kAvg, true, 1u << kMx8, "its sums are taken over every client of an element; use FA_SHARD_RANGE",
     " (the stage sums the updates of an FA_FEDAVG part)"},
    {"mx8 sum", "MX8-sum", kAvg, true, 1u << kMx8, "its sums are taken over every client of an element; use FA_SHARD_RANGE",
     " (the stage sums the updates of an FA_FEDAVG part)"},
    {"lowrank sum", "low-rank-sum", kAvg, true, 1u << kMx8, "its sums are taken over every client of an element; use FA_SHARD_RANGE",
     " (the stage sums the updates of an FA_FEDAVG part)"},
    {"rot1 sum", "rot1-sum", kAvg, true, 1u << kMx8, "its sums are taken over every client of an element; use FA_SHARD_RANGE",
     " (the stage sums the updates of an FA_FEDAVG part)"},
};

// The request "turn stage id on (or off), on the context default (part_id < 0, *out = null) or on this part (*out)"
// against the table, in the order the setters have always checked: the context, the rs refusal (only when turning on:
// turning off is accepted on any context), the part, and when turning on its mode and the family.
int admit(fa_ctx* ctx, StageId id, bool on, int part_id, Part** out) {
    static const char* const kModeName[] = {"FA_FEDAVG", "FA_LITERAL", "FA_TRIMMED"};
    const StageRule& r = kRules[id];
    *out = nullptr;
    if (!ctx) return fail(FA_ERR_ARG, "ctx is null");
    if (on && (ctx->flags & FA_SHARD_CLIENT_RS))
        return fail(FA_ERR_ARG, "%s: not on an FA_SHARD_CLIENT_RS context (%s)", r.name, r.rs_tail);
    if (part_id >= 0)
        if (int rc = check_part(ctx, part_id, out)) return rc;
    const Part* p = *out;
    if (!on) return FA_OK;
    if (p && !(r.modes >> p->mode & 1))
        return fail(FA_ERR_ARG, "%s: part %d is an %s part%s", r.name, part_id, kModeName[p->mode], r.mode_tail);
    const unsigned have = p ? stages_on(*p) : stages_on(ctx->defaults);
    for (int o = 0; r.family && o < kStages; ++o) {
        if (o == id || !kRules[o].family || !(have >> o & 1)) continue;
        if (!p) return fail(FA_ERR_ARG, "%s: the context default has a %s stage (the two stages do not compose)", r.name, kRules[o].title);
        return fail(FA_ERR_ARG, "%s: part %d has a %s stage (the two stages do not compose)", r.name, part_id, kRules[o].title);
    }
    for (int o = 0; p && o < kStages; ++o)  // masked words are no MX8 deltas, and MX8 slots hold no masked words
        if (have & r.never & (1u << o))
            return fail(FA_ERR_ARG, "%s: part %d has a %s stage (the two stages do not compose)", r.name, part_id, kRules[o].title);
    if ((id == kOpt || id == kNoise) && p && p->sign.on() && p->sign.cfg.planes)
        return fail(FA_ERR_STATE, "%s: part %d leaves vote planes (fa_set_sign): its reply would be no function of them", r.name, part_id);
    if (id == kSecagg && p && p->in != FA_F32)
        return fail(FA_ERR_ARG, "secagg: part %d has %s slots (masked uint32 words lie in FA_F32 slots)", part_id, fa::dtype_name(p->in));
    if (id == kSecagg && p && (uint64_t)p->n > kSecaggMaxIndex)
        return fail(FA_ERR_ARG, "secagg: part %d holds more than 2^36 elements (the ChaCha20 block counter has 32 bits)", part_id);
    return FA_OK;
}

// The check of a stage's numbers against a part's D clients, for the stages that have one (Krum's m = -1 is resolved).
int check_for_clients(StageId id, int D, StageCfgs& c) {
    if (id == kKrum) return check_krum(D, c.krum.f, c.krum.m, &c.krum.m);
    if (id == kGeomed) return check_geomed(D, c.geomed.iters, c.geomed.nu);
    if (id == kDnc) return check_dnc(D, c.dnc.drop, c.dnc.iters);
    if (id == kSign) return check_sign_clients(D, c.sign.margin);
    if (id == kSparse) return check_sparse_clients(D);
    if (id == kMx8Sum) return check_mx8sum_clients(D);
    if (id == kLowrankSum) return check_lrsum_clients(D);
    if (id == kRot1Sum) return check_rot1sum_clients(D);
    return id == kBulyan ? check_bulyan(D, c.bulyan.f) : FA_OK;
}

// What every fa_set_* does once the stage's own numbers are checked.  c: the context's defaults with the request in
// place of stage id's (requested) -- the new defaults as they stand, or what set_part_stage applies to the part.
StageCfgs requested(const fa_ctx* ctx) { return ctx ? ctx->defaults : StageCfgs{}; }
int set_stage(fa_ctx* ctx, int part_id, StageId id, StageCfgs c) {
    const bool on = stages_on(c) >> id & 1;
    Part* p;
    if (int rc = admit(ctx, id, on, part_id, &p)) return rc;
    if (!p) {
        ctx->defaults = c;
        return FA_OK;
    }
    if (on)
        if (int rc = check_for_clients(id, p->D, c)) return rc;
    return set_part_stage(ctx, *p, id, c);
}

int taken_defaults(const fa_ctx* ctx, fa_mode mode, int D, StageCfgs* c, unsigned* taken) {
    *c = ctx->defaults;
    *taken = 0;
    for (int id = 0; id < kStages && !(ctx->flags & FA_SHARD_CLIENT_RS); ++id) {
        if (!(stages_on(*c) >> id & 1) || !(kRules[id].modes >> mode & 1)) continue;
        if (int rc = check_for_clients((StageId)id, D, *c)) return rc;
        *taken |= 1u << id;
    }
    return FA_OK;
}

// The prologue of the entries that read or write a part's stage: the part, and that it has stage id; for the four
// reports also that a reducing call ran with it.
int stage_part(fa_ctx* ctx, int part_id, StageId id, Part** out, bool report = false) {
    if (int rc = check_part(ctx, part_id, out)) return rc;
    const Part& p = **out;
    if (!(stages_on(p) >> id & 1)) return fail(FA_ERR_STATE, "part %d has no %s stage", part_id, kRules[id].title);
    if (report && !(id == kClip ? p.clip.reported : id == kKrum ? p.krum.reported : id == kGeomed ? p.geomed.reported :
                    id == kDnc ? p.dnc.reported : p.bulyan.reported))
        return fail(FA_ERR_STATE, "part %d: no round reduced with the %s stage yet", part_id, kRules[id].title);
    return FA_OK;
}

// ------------------------------------------------------------------ MX8 receipts (fa.h "MX8 receipts")

// The scale bytes GPU g's range [off, off + cnt) touches: blocks off >> 5 .. (off + cnt - 1) >> 5.
inline size_t mx8_scales(size_t off, size_t cnt) { return cnt ? ((off + cnt - 1) >> 5) - (off >> 5) + 1 : 0; }

// The MX8 shadow layout, per GPU (the MX8 receipts' and the MX8-sum stage's): q, cnt bytes rounded up to 16, then the
// scale bytes of the blocks the range touches; the stride between slots rounded up to 256.
void mx8_shadow_layout(const Part& p, int G, std::vector<size_t>* stride, std::vector<size_t>* eoff) {
    stride->clear();
    eoff->clear();
    for (size_t g = 0; g < (size_t)G; ++g) {
        eoff->push_back((p.cnt[g] + 15) / 16 * 16);
        stride->push_back(((*eoff)[g] + mx8_scales(p.off[g], p.cnt[g]) + 255) / 256 * 256);
    }
}

// The shadows of an MX8 part, allocated once: per GPU held x stride bytes.  q lies at the shadow's start, which
// keeps the 16-byte phase of the slots and the output (all 16-byte aligned: the vector form applies).  On failure the
// part stays an MX8 part.
int ensure_mx8_buf(fa_ctx* ctx, Part& p) {
    Mx8Stage& s = p.mx8;
    if (s.buf) return FA_OK;
    mx8_shadow_layout(p, ctx->G, &s.stride, &s.eoff);
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.stride[g]); };
    const int g = s.buf.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "mx8: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

// H2D of `bytes` host bytes into dev on GPU r's copy stream: straight from pinned memory, else through the pinned
// chunks, double-buffered as a pageable submit.
int mx8_h2d(GpuRes& r, char* dev, const char* src, size_t bytes, bool pinned) {
    if (pinned) {
        if (bytes) FA_HIP(hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, r.copy));
        return FA_OK;
    }
    for (size_t o = 0; o < bytes; o += kStageBytes) {
        const size_t b = std::min(kStageBytes, bytes - o);
        const int i = r.stage_i;
        r.stage_i ^= 1;
        FA_HIP(hipEventSynchronize(r.stage_ev[i]));
        r.pool->copy(r.stage[i], b, [&](size_t lo, size_t len, char* d) { std::memcpy(d, src + o + lo, len); });
        FA_HIP(hipMemcpyAsync(dev + o, r.stage[i], b, hipMemcpyHostToDevice, r.copy));
        FA_HIP(hipEventRecord(r.stage_ev[i], r.copy));
    }
    return FA_OK;
}

int submit_mx8_impl(fa_ctx* ctx, int part_id, int slot, const int8_t* q, const uint8_t* e, float weight, int flags) {
    Trace tr("fa_submit_mx8 part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~(FA_HOST_PINNED | FA_MX8_ABSOLUTE)) return fail(FA_ERR_ARG, "mx8: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    if (!p->mx8.cfg.flag) return fail(FA_ERR_STATE, "mx8: part %d does not take MX8 receipts (fa_set_mx8)", part_id);
    if (p->n > 0 && (!q || !e)) return fail(FA_ERR_ARG, "mx8: %s is null", !q ? "q" : "e");
    const bool pinned = (flags & FA_HOST_PINNED) != 0, absolute = (flags & FA_MX8_ABSOLUTE) != 0;
    if (!absolute && !p->mx8.ref)
        return fail(FA_ERR_STATE, "mx8: part %d has no reference (no round reduced with fa_set_mx8 on, no "
                                  "fa_mx8_set_reference): send a full receipt, or FA_MX8_ABSOLUTE", part_id);
    if ((rc = ensure_mx8_buf(ctx, *p))) return rc;
    if ((rc = host_flush(ctx, *p))) return rc;  // none is kept while mx8 is on; the plain path from here on
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        const size_t off = p->off[(size_t)g], cnt = p->cnt[(size_t)g];
        if (cnt == 0) return FA_OK;
        // after the part's last reducing call: it read the slot and wrote the reference
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.copy, p->done[(size_t)g], 0));
        }
        char* dq = p->mx8.buf.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * p->mx8.stride[(size_t)g];
        char* de = dq + p->mx8.eoff[(size_t)g];
        ++r.copy_gen;  // the next reducing call waits for the copy stream: the copies and the expansion
        int rc2 = mx8_h2d(r, dq, reinterpret_cast<const char*>(q) + off, cnt, pinned);
        if (!rc2) rc2 = mx8_h2d(r, de, reinterpret_cast<const char*>(e) + (off >> 5), mx8_scales(off, cnt), pinned);
        if (rc2) return rc2;
        for (int j = 0; j < p->npiece[(size_t)g]; ++j) {
            const size_t lo = piece_lo(*p, g, j), pc = piece_cnt(*p, g, j);
            const void* ref = absolute ? nullptr : static_cast<const char*>(p->dout[(size_t)g]) + lo * dsize(p->out);
            FA_HIP(fa::launch_mx8_expand(reinterpret_cast<const int8_t*>(dq) + lo,
                                         reinterpret_cast<const uint8_t*>(de) + (((off + lo) >> 5) - (off >> 5)),
                                         (uint64_t)(off + lo), (int64_t)pc, ref, p->out, piece_ptr(*p, g, slot, j), p->in,
                                         r.copy));
        }
        return FA_OK;
    });
    if (rc) return rc;
    return mark_submitted(ctx, *p, slot, weight);
}

// ------------------------------------------------------------------ top-k receipts (fa.h "Top-k receipts")

// The sparse shadows of a part, allocated once per k_max: per GPU held x sstride bytes, a shadow scap[g] = min(k_max,
// cnt) indices followed by as many values.  On failure the part keeps the stage.
int ensure_topk_buf(fa_ctx* ctx, Part& p) {
    Mx8Stage& s = p.mx8;
    if (s.sparse) return FA_OK;
    s.scap.clear();
    s.sstride.clear();
    for (size_t g = 0; g < (size_t)ctx->G; ++g) {
        s.scap.push_back(std::min(s.cfg.k_max, p.cnt[g]));
        s.sstride.push_back((s.scap[g] * 8 + 255) / 256 * 256);
    }
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.sstride[g]); };
    const int g = s.sparse.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "topk: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

int submit_topk_impl(fa_ctx* ctx, int part_id, int slot, const uint32_t* idx, const float* val, size_t k, float weight,
                     int flags) {
    Trace tr("fa_submit_topk part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~(FA_HOST_PINNED | FA_TOPK_ABSOLUTE)) return fail(FA_ERR_ARG, "topk: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    if (!p->mx8.cfg.k_max) return fail(FA_ERR_STATE, "topk: part %d does not take top-k receipts (fa_set_topk)", part_id);
    if (k > p->mx8.cfg.k_max) return fail(FA_ERR_ARG, "topk: %zu entries, part %d takes at most %zu (fa_set_topk)", k, part_id, p->mx8.cfg.k_max);
    if (k && (!idx || !val)) return fail(FA_ERR_ARG, "topk: %s is null", !idx ? "idx" : "val");
    if (k && (uint64_t)p->n > (1ull << 32)) return fail(FA_ERR_ARG, "topk: part %d holds more than 2^32 elements", part_id);
    for (size_t j = 0; j < k; ++j) {
        if ((uint64_t)idx[j] >= (uint64_t)p->n) return fail(FA_ERR_ARG, "topk: idx[%zu] = %u, the bucket holds %zu elements", j, idx[j], p->n);
        if (j && idx[j] <= idx[j - 1])
            return fail(FA_ERR_ARG, "topk: idx[%zu] = %u after idx[%zu] = %u: not strictly ascending", j, idx[j], j - 1, idx[j - 1]);
    }
    const bool pinned = (flags & FA_HOST_PINNED) != 0, absolute = (flags & FA_TOPK_ABSOLUTE) != 0;
    if (!absolute && !p->mx8.ref)
        return fail(FA_ERR_STATE, "topk: part %d has no reference (no round reduced with the stage on, no "
                                  "fa_mx8_set_reference): send a full receipt, or FA_TOPK_ABSOLUTE", part_id);
    if ((rc = ensure_topk_buf(ctx, *p))) return rc;
    if ((rc = host_flush(ctx, *p))) return rc;  // none is kept while the stage is on; the plain path from here on
    const auto first_at = [&](size_t e) { return (size_t)(std::lower_bound(idx, idx + k, (uint64_t)e, [](uint32_t a, uint64_t b) { return (uint64_t)a < b; }) - idx); };
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        const size_t off = p->off[(size_t)g], cnt = p->cnt[(size_t)g];
        if (cnt == 0) return FA_OK;
        // after the part's last reducing call: it read the slot and wrote the reference
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.copy, p->done[(size_t)g], 0));
        }
        const size_t a = first_at(off), b = first_at(off + cnt);  // the GPU's entries: b - a <= min(k_max, cnt)
        char* di = p->mx8.sparse.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * p->mx8.sstride[(size_t)g];
        char* dv = di + p->mx8.scap[(size_t)g] * 4;
        ++r.copy_gen;  // the next reducing call waits for the copy stream: the copies and the expansion
        int rc2 = mx8_h2d(r, di, reinterpret_cast<const char*>(idx + a), (b - a) * 4, pinned);
        if (!rc2) rc2 = mx8_h2d(r, dv, reinterpret_cast<const char*>(val + a), (b - a) * 4, pinned);
        if (rc2) return rc2;
        for (int j = 0; j < p->npiece[(size_t)g]; ++j) {
            const size_t lo = piece_lo(*p, g, j), pc = piece_cnt(*p, g, j);
            const size_t pa = first_at(off + lo) - a, pb = first_at(off + lo + pc) - a;
            const void* ref = absolute ? nullptr : static_cast<const char*>(p->dout[(size_t)g]) + lo * dsize(p->out);
            FA_HIP(fa::launch_topk_expand(reinterpret_cast<const uint32_t*>(di) + pa, reinterpret_cast<const float*>(dv) + pa,
                                          (uint64_t)(pb - pa), (uint64_t)(off + lo), (int64_t)pc, ref, p->out,
                                          piece_ptr(*p, g, slot, j), p->in, r.copy));
        }
        return FA_OK;
    });
    if (rc) return rc;
    return mark_submitted(ctx, *p, slot, weight);
}

// ------------------------------------------------------------------ low-rank receipts (fa.h "Low-rank receipts")

// The factor shadows of a part, allocated once per table and r_max: per GPU held x fstride bytes, a shadow the whole
// receipt at rank r_max.  On failure the part keeps the stage.
int ensure_lowrank_buf(fa_ctx* ctx, Part& p) {
    Mx8Stage& s = p.mx8;
    if (s.factors) return FA_OK;
    s.fstride = ((size_t)fa::lowrank_len(s.cfg.mats.data(), s.cfg.mats.size(), p.n, s.cfg.r_max) * 4 + 255) / 256 * 256;
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.fstride); };
    const int g = s.factors.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "lowrank: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

int submit_lowrank_impl(fa_ctx* ctx, int part_id, int slot, const float* f, size_t len, int r, float weight, int flags) {
    Trace tr("fa_submit_lowrank part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~(FA_HOST_PINNED | FA_LOWRANK_ABSOLUTE)) return fail(FA_ERR_ARG, "lowrank: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    const ReceiptCfg& c = p->mx8.cfg;
    if (!c.lowrank()) return fail(FA_ERR_STATE, "lowrank: part %d does not take low-rank receipts (fa_set_lowrank)", part_id);
    if (r < 1 || r > c.r_max) return fail(FA_ERR_ARG, "lowrank: rank %d, part %d takes 1 .. %d (fa_set_lowrank)", r, part_id, c.r_max);
    const size_t need = (size_t)fa::lowrank_len(c.mats.data(), c.mats.size(), p->n, r);
    if (len != need) return fail(FA_ERR_ARG, "lowrank: %zu values, a receipt of rank %d for part %d has %zu (fa_lowrank_len)", len, r, part_id, need);
    if (len && !f) return fail(FA_ERR_ARG, "lowrank: f is null");
    const bool pinned = (flags & FA_HOST_PINNED) != 0, absolute = (flags & FA_LOWRANK_ABSOLUTE) != 0;
    if (!absolute && !p->mx8.ref)
        return fail(FA_ERR_STATE, "lowrank: part %d has no reference (no round reduced with the stage on, no "
                                  "fa_mx8_set_reference): send a full receipt, or FA_LOWRANK_ABSOLUTE", part_id);
    if ((rc = ensure_lowrank_buf(ctx, *p))) return rc;
    if ((rc = host_flush(ctx, *p))) return rc;  // none is kept while the stage is on; the plain path from here on
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& gr = ctx->gpu[(size_t)g];
        DeviceGuard dg(gr.dev);
        const size_t off = p->off[(size_t)g], cnt = p->cnt[(size_t)g];
        if (cnt == 0) return FA_OK;
        // after the part's last reducing call: it read the slot and wrote the reference
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(gr.copy, p->done[(size_t)g], 0));
        }
        char* df = p->mx8.factors.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * p->mx8.fstride;
        ++gr.copy_gen;  // the next reducing call waits for the copy stream: the copy and the expansion
        if (int rc2 = mx8_h2d(gr, df, reinterpret_cast<const char*>(f), len * 4, pinned)) return rc2;
        for (int j = 0; j < p->npiece[(size_t)g]; ++j) {
            const size_t lo = piece_lo(*p, g, j), pc = piece_cnt(*p, g, j);
            const void* ref = absolute ? nullptr : static_cast<const char*>(p->dout[(size_t)g]) + lo * dsize(p->out);
            FA_HIP(fa::launch_lowrank_expand(p->mx8.plan.at((size_t)g) + p->mx8.plan_at[(size_t)g][(size_t)j],
                                             p->mx8.plan_len[(size_t)g][(size_t)j], reinterpret_cast<const float*>(df), r,
                                             (uint64_t)(off + lo), (int64_t)pc, ref, p->out, piece_ptr(*p, g, slot, j), p->in,
                                             gr.copy));
        }
        return FA_OK;
    });
    if (rc) return rc;
    return mark_submitted(ctx, *p, slot, weight);
}

// ------------------------------------------------------------------ rot1 receipts (fa.h "Rot1 receipts")

// The blocks of 4096 elements GPU g's range [off, off + cnt) touches: off >> 12 .. (off + cnt - 1) >> 12.
inline size_t rot1_blocks(size_t off, size_t cnt) { return cnt ? ((off + cnt - 1) >> 12) - (off >> 12) + 1 : 0; }

// The rot1 shadow layout, per GPU (the rot1 receipts' and the rot1-sum stage's): the words of the blocks the GPU's range
// touches, then from soff on their scales, 516 bytes per block; the stride between slots rounded up to 256.
void rot1_shadow_layout(const Part& p, int G, std::vector<size_t>* stride, std::vector<size_t>* soff) {
    stride->clear();
    soff->clear();
    for (size_t g = 0; g < (size_t)G; ++g) {
        const size_t nb = rot1_blocks(p.off[g], p.cnt[g]);
        soff->push_back(nb * fa::kRot1Words * 4);
        stride->push_back((nb * (fa::kRot1Words + 1) * 4 + 255) / 256 * 256);
    }
}

// The rot1 shadows of a part, allocated once: per GPU held x rstride bytes in the rot1 shadow layout.  On failure the
// part keeps the stage.
int ensure_rot1_buf(fa_ctx* ctx, Part& p) {
    Mx8Stage& s = p.mx8;
    if (s.rot) return FA_OK;
    rot1_shadow_layout(p, ctx->G, &s.rstride, &s.rsoff);
    const auto bytes = [&](size_t g) { return std::max<size_t>(256, (size_t)(p.c1[g] - p.c0[g]) * s.rstride[g]); };
    const int g = s.rot.alloc(ctx->gpu, bytes);
    if (g < 0) return FA_OK;
    return fail(FA_ERR_NOMEM, "rot1: shadow alloc of %zu B failed on GPU %zu", bytes((size_t)g), (size_t)g);
}

int submit_rot1_impl(fa_ctx* ctx, int part_id, int slot, const uint32_t* bits, const float* scale, uint64_t seed,
                     float weight, int flags) {
    Trace tr("fa_submit_rot1 part %d slot %d", part_id, slot);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (flags & ~(FA_HOST_PINNED | FA_ROT1_ABSOLUTE)) return fail(FA_ERR_ARG, "rot1: unknown flags 0x%x", flags);
    if (slot < 0 || slot >= p->D) return fail(FA_ERR_ARG, "client slot %d out of range [0,%d)", slot, p->D);
    if (!p->mx8.cfg.rot1) return fail(FA_ERR_STATE, "rot1: part %d does not take rot1 receipts (fa_set_rot1)", part_id);
    if (p->n > 0 && (!bits || !scale)) return fail(FA_ERR_ARG, "rot1: %s is null", !bits ? "bits" : "scale");
    const bool pinned = (flags & FA_HOST_PINNED) != 0, absolute = (flags & FA_ROT1_ABSOLUTE) != 0;
    if (!absolute && !p->mx8.ref)
        return fail(FA_ERR_STATE, "rot1: part %d has no reference (no round reduced with the stage on, no "
                                  "fa_mx8_set_reference): send a full receipt, or FA_ROT1_ABSOLUTE", part_id);
    if ((rc = ensure_rot1_buf(ctx, *p))) return rc;
    if ((rc = host_flush(ctx, *p))) return rc;  // none is kept while the stage is on; the plain path from here on
    rc = for_each_gpu(ctx->workers.get(), ctx->G, [&](int g) -> int {
        GpuRes& r = ctx->gpu[(size_t)g];
        DeviceGuard dg(r.dev);
        const size_t off = p->off[(size_t)g], cnt = p->cnt[(size_t)g];
        if (cnt == 0) return FA_OK;
        // after the part's last reducing call: it read the slot and wrote the reference
        if (hipStream_t ds = p->done_stream[(size_t)g]) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.copy, p->done[(size_t)g], 0));
        }
        const size_t b0 = off >> 12, nb = rot1_blocks(off, cnt);
        char* db = p->mx8.rot.at((size_t)g) + (size_t)(slot - p->c0[(size_t)g]) * p->mx8.rstride[(size_t)g];
        char* dsc = db + p->mx8.rsoff[(size_t)g];
        ++r.copy_gen;  // the next reducing call waits for the copy stream: the copies and the expansion
        int rc2 = mx8_h2d(r, db, reinterpret_cast<const char*>(bits + b0 * fa::kRot1Words), nb * fa::kRot1Words * 4, pinned);
        if (!rc2) rc2 = mx8_h2d(r, dsc, reinterpret_cast<const char*>(scale + b0), nb * 4, pinned);
        if (rc2) return rc2;
        for (int j = 0; j < p->npiece[(size_t)g]; ++j) {
            const size_t lo = piece_lo(*p, g, j), pc = piece_cnt(*p, g, j);
            if (pc == 0) continue;
            const size_t pb = ((off + lo) >> 12) - b0;  // the piece's first block among the GPU's
            const void* ref = absolute ? nullptr : static_cast<const char*>(p->dout[(size_t)g]) + lo * dsize(p->out);
            FA_HIP(fa::launch_rot1_expand(reinterpret_cast<const uint32_t*>(db) + pb * fa::kRot1Words,
                                          reinterpret_cast<const float*>(dsc) + pb, seed, (uint64_t)(off + lo), (int64_t)pc,
                                          ref, p->out, piece_ptr(*p, g, slot, j), p->in, r.copy));
        }
        return FA_OK;
    });
    if (rc) return rc;
    return mark_submitted(ctx, *p, slot, weight);
}

// The receipt formats a fa_set_mx8 / fa_set_topk / fa_set_lowrank / fa_set_rot1 starts from: the part's own, or the context default's.
ReceiptCfg receipts_of(fa_ctx* ctx, int part_id) {
    if (!ctx) return ReceiptCfg{};
    const auto it = ctx->parts.find(part_id);
    return part_id >= 0 && it != ctx->parts.end() ? it->second.mx8.cfg : ctx->defaults.mx8;
}

}  // namespace fah

using namespace fah;

extern "C" {

int fa_set_server_opt(fa_ctx* ctx, int part_id, const fa_server_opt* opt) {
    g_err.clear();
    if (!ctx) return fail(FA_ERR_ARG, "ctx is null");
    StageCfgs c = requested(ctx);
    c.opt = opt ? OptCfg(*opt) : OptCfg();
    if (int rc = check_opt(c.opt)) return rc;
    return set_stage(ctx, part_id, kOpt, c);
}

int fa_server_opt_set_state(fa_ctx* ctx, int part_id, const float* x, const float* m, const float* v, uint64_t steps) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kOpt, &p);
    if (rc) return rc;
    if ((rc = wait_devices(ctx))) return rc;
    for (int g = 0; g < ctx->G; ++g) {
        DeviceGuard dg(ctx->gpu[(size_t)g].dev);
        const size_t off = p->off[(size_t)g], bytes = p->cnt[(size_t)g] * 4;
        if (!bytes) continue;
        if (x) FA_HIP(hipMemcpy(p->opt.x.at<float>((size_t)g), x + off, bytes, hipMemcpyHostToDevice));
        if (m) FA_HIP(hipMemcpy(p->opt.m.at<float>((size_t)g), m + off, bytes, hipMemcpyHostToDevice));
        if (v && opt_adaptive(p->opt.cfg.rule)) FA_HIP(hipMemcpy(p->opt.v.at<float>((size_t)g), v + off, bytes, hipMemcpyHostToDevice));
    }
    if ((rc = wait_devices(ctx))) return rc;  // the copies land before any later launch on the ctx streams
    if (x) p->opt.master = true;
    p->opt.steps = steps;
    return FA_OK;
}

int fa_server_opt_get_state(fa_ctx* ctx, int part_id, float* x, float* m, float* v, uint64_t* steps) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kOpt, &p);
    if (rc) return rc;
    if (steps) *steps = p->opt.steps;
    if (!x && !m && !v) return FA_OK;  // the step count alone is host state: no device wait
    if ((rc = wait_devices(ctx))) return rc;
    for (int g = 0; g < ctx->G; ++g) {
        DeviceGuard dg(ctx->gpu[(size_t)g].dev);
        const size_t off = p->off[(size_t)g], bytes = p->cnt[(size_t)g] * 4;
        if (!bytes) continue;
        if (x) FA_HIP(hipMemcpy(x + off, p->opt.x.at<float>((size_t)g), bytes, hipMemcpyDeviceToHost));
        if (m) FA_HIP(hipMemcpy(m + off, p->opt.m.at<float>((size_t)g), bytes, hipMemcpyDeviceToHost));
        if (v && opt_adaptive(p->opt.cfg.rule)) FA_HIP(hipMemcpy(v + off, p->opt.v.at<float>((size_t)g), bytes, hipMemcpyDeviceToHost));
    }
    return FA_OK;
}

int fa_get_server_opt(fa_ctx* ctx, int part_id, fa_server_opt* opt) {
    g_err.clear();
    if (!ctx || !opt) return fail(FA_ERR_ARG, "ctx or opt is null");
    Part* p = nullptr;
    if (part_id >= 0)
        if (int rc = check_part(ctx, part_id, &p)) return rc;
    *opt = p ? p->opt.cfg : ctx->defaults.opt;
    return FA_OK;
}

int fa_server_opt_device(fa_ctx* ctx, int gpu, const fa_server_opt* opt, const float* d_avg, float* d_x, float* d_m,
                         float* d_v, size_t n, void* d_out, fa_dtype out, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!opt) return fail(FA_ERR_ARG, "server opt: opt is null");
    if (int rc = check_opt(*opt)) return rc;
    if (opt->rule == FA_OPT_NONE) return fail(FA_ERR_ARG, "server opt: rule FA_OPT_NONE takes no step");
    if (!dvalid(out)) return fail(FA_ERR_ARG, "bad dtype");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    const bool needs_v = opt_adaptive(opt->rule);
    if (!d_avg || !d_x || !d_m || (needs_v && !d_v))
        return fail(FA_ERR_ARG, "server opt: %s pointer is null", !d_avg ? "d_avg" : !d_x ? "d_x" : !d_m ? "d_m" : "d_v");
    if (!aligned(d_avg, 4) || !aligned(d_x, 4) || !aligned(d_m, 4) || (needs_v && !aligned(d_v, 4)))
        return fail(FA_ERR_ALIGN, "server opt: aggregate or state not 4-byte aligned");
    if (d_out && !aligned(d_out, dsize(out))) return fail(FA_ERR_ALIGN, "output not %zu-byte aligned", dsize(out));
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    return opt_on(c.tu, opt->rule, *opt, d_avg, d_x, d_m, needs_v ? d_v : nullptr, n, d_out, out, c.s);
}

int fa_set_clip(fa_ctx* ctx, int part_id, float max_norm) {
    g_err.clear();
    if (!finite_f(max_norm) || max_norm < 0.0f)
        return fail(FA_ERR_ARG, "clip: max_norm %g must be finite and >= 0", (double)max_norm);
    StageCfgs c = requested(ctx);
    c.clip.max_norm = max_norm;
    return set_stage(ctx, part_id, kClip, c);
}

int fa_clip_set_reference(fa_ctx* ctx, int part_id, const float* g) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kClip, &p);
    if (rc) return rc;
    if ((rc = wait_devices(ctx))) return rc;
    for (int gi = 0; g && gi < ctx->G; ++gi) {
        DeviceGuard dg(ctx->gpu[(size_t)gi].dev);
        const size_t bytes = p->cnt[(size_t)gi] * 4;
        if (bytes) FA_HIP(hipMemcpy(p->clip.ref.at<float>((size_t)gi), g + p->off[(size_t)gi], bytes, hipMemcpyHostToDevice));
    }
    if (g && (rc = wait_devices(ctx))) return rc;  // the copies land before any later launch on the ctx streams
    p->clip.has_ref = g != nullptr;
    return FA_OK;
}

int fa_clip_get_reference(fa_ctx* ctx, int part_id, float* g) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kClip, &p);
    if (rc) return rc;
    if (!p->clip.has_ref) return fail(FA_ERR_STATE, "part %d has no clip reference yet", part_id);
    if (!g && p->n) return fail(FA_ERR_ARG, "g is null");
    if ((rc = wait_devices(ctx))) return rc;
    for (int gi = 0; gi < ctx->G; ++gi) {
        DeviceGuard dg(ctx->gpu[(size_t)gi].dev);
        const size_t bytes = p->cnt[(size_t)gi] * 4;
        if (bytes) FA_HIP(hipMemcpy(g + p->off[(size_t)gi], p->clip.ref.at<float>((size_t)gi), bytes, hipMemcpyDeviceToHost));
    }
    return FA_OK;
}

int fa_clip_get_round(fa_ctx* ctx, int part_id, double* sumsq, float* scales, int* included, int* n_clipped) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kClip, &p, true);
    if (rc) return rc;
    for (size_t k = 0; k < (size_t)p->D; ++k) {
        if (sumsq) sumsq[k] = p->clip.q[k];
        if (scales) scales[k] = p->clip.in[k] ? p->clip.s[k] : 0.0f;
        if (included) included[k] = p->clip.in[k];
    }
    if (n_clipped) *n_clipped = p->clip.n;
    return FA_OK;
}

float fa_clip_scale(double sumsq, float max_norm, int* excluded) { return clip_scale(sumsq, max_norm, excluded); }

int fa_clip_sumsq_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in,
                         const float* d_ref, double* h_sumsq, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (D < 1) return fail(FA_ERR_ARG, "clip: D must be >= 1");
    if (!dvalid(in)) return fail(FA_ERR_ARG, "bad dtype");
    if (!h_sumsq) return fail(FA_ERR_ARG, "clip: h_sumsq is null");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) {
        std::fill(h_sumsq, h_sumsq + D, 0.0);
        return FA_OK;
    }
    if (int rc = check_clients(d_clients, D, dsize(in), "client")) return rc;
    if (!d_ref) return fail(FA_ERR_ARG, "clip: d_ref is null");
    if (!aligned(d_ref, 4)) return fail(FA_ERR_ALIGN, "clip: reference not 4-byte aligned");
    return measure_device(ctx, gpu, hip_stream, (size_t)D, kClipParts, "clip: norm-pass", h_sumsq,
                          [&](const DeviceCall& c, double* d_part, double* d_out) {
                              return clip_sumsq_on(c.tu, d_clients, D, n, in, d_ref, d_part, d_out, c.s);
                          });
}

int fa_set_krum(fa_ctx* ctx, int part_id, int f, int m) {
    g_err.clear();
    if (f < 0 || m < -1) return fail(FA_ERR_ARG, "krum: f = %d, m = %d (f >= 0; m >= 1, -1 for D - f, 0 removes the stage)", f, m);
    StageCfgs c = requested(ctx);
    c.krum = KrumCfg{m != 0 ? f : 0, m};
    return set_stage(ctx, part_id, kKrum, c);
}

int fa_krum_get_round(fa_ctx* ctx, int part_id, double* dist, double* scores, int* selected, int* n_selected) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kKrum, &p, true);
    if (rc) return rc;
    const size_t D = (size_t)p->D;
    if (dist) std::copy(p->krum.q.begin(), p->krum.q.end(), dist);
    for (size_t k = 0; k < D; ++k) {
        if (scores) scores[k] = p->krum.s[k];
        if (selected) selected[k] = p->krum.sel[k];
    }
    if (n_selected) *n_selected = p->krum.n;
    return FA_OK;
}

int fa_krum_select(const double* dist, int D, int f, int m, double* scores, int* selected, int* n_selected) {
    g_err.clear();
    if (!dist) return fail(FA_ERR_ARG, "krum: dist is null");
    if (D < 1) return fail(FA_ERR_ARG, "krum: D must be >= 1");
    int mm = 0;
    if (int rc = check_krum(D, f, m, &mm)) return rc;
    krum_select(dist, D, f, mm, scores, selected, n_selected);
    return FA_OK;
}

int fa_krum_weights(const float* w, const int* selected, int D, float* w_out) {
    g_err.clear();
    if (!w || !selected || !w_out) return fail(FA_ERR_ARG, "krum: w, selected or w_out is null");
    if (D < 1) return fail(FA_ERR_ARG, "krum: D must be >= 1");
    krum_weights(w, selected, D, w_out);
    return FA_OK;
}

int fa_pairdist_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in, double* h_dist,
                       void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (D < 1 || D > FA_KRUM_MAX_CLIENTS) return fail(FA_ERR_ARG, "krum: D = %d outside 1..%d", D, FA_KRUM_MAX_CLIENTS);
    if (!dvalid(in)) return fail(FA_ERR_ARG, "bad dtype");
    if (!h_dist) return fail(FA_ERR_ARG, "krum: h_dist is null");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    const size_t DD = (size_t)D * (size_t)D;
    if (n == 0) {
        std::fill(h_dist, h_dist + DD, 0.0);
        return FA_OK;
    }
    if (int rc = check_clients(d_clients, D, dsize(in), "client")) return rc;
    return measure_device(ctx, gpu, hip_stream, DD, krum_parts(D), "krum: distance-pass", h_dist,
                          [&](const DeviceCall& c, double* d_part, double* d_out) {
                              return pairdist_on(c.tu, d_clients, D, n, in, d_part, d_out, c.s);
                          });
}

int fa_gram_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in, const float* d_ref,
                   double* h_gram, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (D < 1 || D > FA_DNC_MAX_CLIENTS) return fail(FA_ERR_ARG, "gram: D = %d outside 1..%d", D, FA_DNC_MAX_CLIENTS);
    if (!dvalid(in)) return fail(FA_ERR_ARG, "bad dtype");
    if (!h_gram) return fail(FA_ERR_ARG, "gram: h_gram is null");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    const size_t DD = (size_t)D * (size_t)D;
    if (n == 0) {
        std::fill(h_gram, h_gram + DD, 0.0);
        return FA_OK;
    }
    if (int rc = check_clients(d_clients, D, dsize(in), "client")) return rc;
    if (d_ref && !aligned(d_ref, 4)) return fail(FA_ERR_ALIGN, "gram: reference not 4-byte aligned");
    return measure_device(ctx, gpu, hip_stream, DD, gram_parts(D), "gram: gram-pass", h_gram,
                          [&](const DeviceCall& c, double* d_part, double* d_out) {
                              return gram_on(c.tu, d_clients, D, n, in, d_ref, d_part, d_out, c.s);
                          });
}

int fa_set_dnc(fa_ctx* ctx, int part_id, int drop, int iters) {
    g_err.clear();
    if (drop < 0 || iters < 0 || iters > FA_DNC_MAX_ITERS)
        return fail(FA_ERR_ARG, "dnc: drop = %d, iters = %d (drop >= 0; 1 <= iters <= %d, 0 removes the stage)", drop, iters,
                    FA_DNC_MAX_ITERS);
    StageCfgs c = requested(ctx);
    c.dnc = DncCfg{iters != 0 ? drop : 0, iters};
    return set_stage(ctx, part_id, kDnc, c);
}

int fa_dnc_get_round(fa_ctx* ctx, int part_id, double* gram, double* scores, int* selected, int* n_selected) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kDnc, &p, true);
    if (rc) return rc;
    const size_t D = (size_t)p->D;
    if (gram) std::copy(p->dnc.q.begin(), p->dnc.q.end(), gram);
    for (size_t k = 0; k < D; ++k) {
        if (scores) scores[k] = p->dnc.s[k];
        if (selected) selected[k] = p->dnc.sel[k];
    }
    if (n_selected) *n_selected = p->dnc.n;
    return FA_OK;
}

int fa_dnc_select(const double* gram, int D, int drop, int iters, double* scores, int* selected, int* n_selected) {
    g_err.clear();
    if (!gram) return fail(FA_ERR_ARG, "dnc: gram is null");
    if (D < 1) return fail(FA_ERR_ARG, "dnc: D must be >= 1");
    if (int rc = check_dnc(D, drop, iters)) return rc;
    dnc_select(gram, D, drop, iters, scores, selected, n_selected);
    return FA_OK;
}

int fa_set_geomed(fa_ctx* ctx, int part_id, int iters, float nu) {
    g_err.clear();
    if (int rc = check_geomed(0, iters, nu)) return rc;
    StageCfgs c = requested(ctx);
    c.geomed = GeomedCfg{iters, iters != 0 ? nu : 0.0f};
    return set_stage(ctx, part_id, kGeomed, c);
}

int fa_get_geomed(fa_ctx* ctx, int part_id, int* iters, float* nu) {
    g_err.clear();
    if (!ctx) return fail(FA_ERR_ARG, "ctx is null");
    Part* p = nullptr;
    if (part_id >= 0)
        if (int rc = check_part(ctx, part_id, &p)) return rc;
    const GeomedCfg& c = p ? p->geomed.cfg : ctx->defaults.geomed;
    if (iters) *iters = c.iters;
    if (nu) *nu = c.nu;
    return FA_OK;
}

int fa_geomed_get_round(fa_ctx* ctx, int part_id, int* n_passes, double* sumsq, float* weights, int* included,
                        double* objective) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kGeomed, &p, true);
    if (rc) return rc;
    const size_t D = (size_t)p->D, np = (size_t)p->geomed.passes;
    if (n_passes) *n_passes = p->geomed.passes;
    if (sumsq) std::copy(p->geomed.q.begin(), p->geomed.q.begin() + (ptrdiff_t)(np * D), sumsq);
    if (weights) std::copy(p->geomed.w.begin(), p->geomed.w.begin() + (ptrdiff_t)((np + 1) * D), weights);
    if (included) std::copy(p->geomed.in.begin(), p->geomed.in.end(), included);
    if (objective) std::copy(p->geomed.obj.begin(), p->geomed.obj.begin() + (ptrdiff_t)np, objective);
    return FA_OK;
}

int fa_geomed_weights(const float* w, const double* sumsq, int* included, int D, float nu, float* w_out) {
    g_err.clear();
    if (!w || !sumsq || !included || !w_out) return fail(FA_ERR_ARG, "geomed: w, sumsq, included or w_out is null");
    if (D < 1) return fail(FA_ERR_ARG, "geomed: D must be >= 1");
    if (!finite_f(nu) || !(nu > 0.0f)) return fail(FA_ERR_ARG, "geomed: nu %g must be finite and > 0", (double)nu);
    geomed_weights(w, sumsq, included, D, nu, w_out, nullptr);
    return FA_OK;
}

int fa_geomed_pass_device(fa_ctx* ctx, int gpu, const void* const* d_clients, const float* h_weights, int D, size_t n,
                          fa_dtype in, float* d_v, double* h_sumsq, double* h_nonfinite, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (D < 1 || D > FA_GEOMED_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "geomed: D = %d outside 1..%d", D, FA_GEOMED_MAX_CLIENTS);
    if (!dvalid(in)) return fail(FA_ERR_ARG, "bad dtype");
    if (!h_weights) return fail(FA_ERR_ARG, "geomed: h_weights is null");
    if (!h_sumsq || !h_nonfinite) return fail(FA_ERR_ARG, "geomed: %s is null", !h_sumsq ? "h_sumsq" : "h_nonfinite");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) {
        std::fill(h_sumsq, h_sumsq + D, 0.0);
        std::fill(h_nonfinite, h_nonfinite + D, 0.0);
        return FA_OK;
    }
    if (int rc = check_clients(d_clients, D, dsize(in), "client")) return rc;
    if (d_v && !aligned(d_v, 4)) return fail(FA_ERR_ALIGN, "geomed: d_v not 4-byte aligned");
    std::vector<double> res(2 * (size_t)D);
    if (int rc = measure_device(ctx, gpu, hip_stream, 2 * (size_t)D, kGeomedParts, "geomed: fused pass", res.data(),
                                [&](const DeviceCall& c, double* d_part, double* d_out) {
                                    return geomed_pass_on(c.tu, d_clients, h_weights, D, n, in, d_v, d_part, d_out, c.s);
                                }))
        return rc;
    std::copy(res.begin(), res.begin() + D, h_sumsq);
    std::copy(res.begin() + D, res.end(), h_nonfinite);
    return FA_OK;
}

int fa_set_bulyan(fa_ctx* ctx, int part_id, int f) {
    g_err.clear();
    if (f < -1) return fail(FA_ERR_ARG, "bulyan: f = %d (f >= 0; -1 removes the stage)", f);
    StageCfgs c = requested(ctx);
    c.bulyan.f = f;
    return set_stage(ctx, part_id, kBulyan, c);
}

int fa_bulyan_get_round(fa_ctx* ctx, int part_id, double* dist, int* order, double* pick_scores, int* selected,
                        int* n_selected) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kBulyan, &p, true);
    if (rc) return rc;
    const size_t D = (size_t)p->D;
    if (dist) std::copy(p->bulyan.q.begin(), p->bulyan.q.end(), dist);
    for (size_t k = 0; k < D; ++k) {
        if (order) order[k] = p->bulyan.order[k];
        if (pick_scores) pick_scores[k] = p->bulyan.s[k];
        if (selected) selected[k] = p->bulyan.sel[k];
    }
    if (n_selected) *n_selected = p->bulyan.n;
    return FA_OK;
}

int fa_bulyan_select(const double* dist, int D, int f, int* order, double* pick_scores, int* selected, int* n_selected) {
    g_err.clear();
    if (!dist) return fail(FA_ERR_ARG, "bulyan: dist is null");
    if (D < 1) return fail(FA_ERR_ARG, "bulyan: D must be >= 1");
    if (int rc = check_bulyan(D, f)) return rc;
    bulyan_select(dist, D, f, order, pick_scores, selected, n_selected);
    return FA_OK;
}

int fa_centered_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in, void* d_out,
                       fa_dtype out, int keep, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (D < 1 || D > FA_TRIMMED_MAX_CLIENTS)
        return fail(FA_ERR_ARG, "D = %d: a centred mean takes 1..%d clients", D, FA_TRIMMED_MAX_CLIENTS);
    if (keep < 1 || keep > D) return fail(FA_ERR_ARG, "keep %d does not fit D = %d clients (1 <= keep <= D)", keep, D);
    if (!dvalid(in) || !dvalid(out)) return fail(FA_ERR_ARG, "bad dtype");
    FA_PAIR(in, out);
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if (int rc = check_clients(d_clients, D, dsize(in), "client")) return rc;
    if (!d_out) return fail(FA_ERR_ARG, "output pointer is null");
    if (!aligned(d_out, dsize(out))) return fail(FA_ERR_ALIGN, "output not %zu-byte aligned", dsize(out));
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    return centered_on(c.tu, d_clients, D, n, in, d_out, out, keep, c.s);
}

int fa_set_noise(fa_ctx* ctx, int part_id, float stddev, uint64_t seed) {
    g_err.clear();
    if (!finite_f(stddev) || stddev < 0.0f) return fail(FA_ERR_ARG, "noise: stddev %g must be finite and >= 0", (double)stddev);
    StageCfgs c = requested(ctx);
    c.noise = NoiseCfg{stddev, stddev > 0.0f ? seed : 0};
    return set_stage(ctx, part_id, kNoise, c);
}

int fa_get_noise(fa_ctx* ctx, int part_id, float* stddev, uint64_t* seed) {
    g_err.clear();
    if (!ctx) return fail(FA_ERR_ARG, "ctx is null");
    Part* p = nullptr;
    if (part_id >= 0)
        if (int rc = check_part(ctx, part_id, &p)) return rc;
    const NoiseCfg& c = p ? p->noise.cfg : ctx->defaults.noise;
    if (stddev) *stddev = c.stddev;
    if (seed) *seed = c.seed;
    return FA_OK;
}

int fa_noise_get_round(fa_ctx* ctx, int part_id, uint64_t* round) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kNoise, &p);
    if (rc) return rc;
    if (!round) return fail(FA_ERR_ARG, "round is null");
    *round = p->noise.round;
    return FA_OK;
}

int fa_noise_set_round(fa_ctx* ctx, int part_id, uint64_t round) {
    g_err.clear();
    Part* p;
    int rc = stage_part(ctx, part_id, kNoise, &p);
    if (rc) return rc;
    if (round > kNoiseRounds) return fail(FA_ERR_ARG, "noise: round %llu beyond 2^32", (unsigned long long)round);
    p->noise.round = round;
    return FA_OK;
}

int fa_noise_device(fa_ctx* ctx, int gpu, const float* d_avg, size_t n, void* d_out, fa_dtype out, float stddev,
                    uint64_t seed, uint32_t stream, uint32_t round, uint64_t idx0, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!finite_f(stddev) || !(stddev > 0.0f)) return fail(FA_ERR_ARG, "noise: stddev %g must be finite and > 0", (double)stddev);
    if (!dvalid(out)) return fail(FA_ERR_ARG, "bad dtype");
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "noise: idx0 + n beyond 2^64");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if (!d_avg || !d_out) return fail(FA_ERR_ARG, "noise: %s pointer is null", !d_avg ? "d_avg" : "d_out");
    if (!aligned(d_avg, 4)) return fail(FA_ERR_ALIGN, "noise: aggregate not 4-byte aligned");
    if (!aligned(d_out, dsize(out))) return fail(FA_ERR_ALIGN, "output not %zu-byte aligned", dsize(out));
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    return noise_on(c.tu, d_avg, d_out, out, stddev, seed, stream, round, idx0, n, c.s);
}

int fa_noise_host(uint64_t seed, uint32_t stream, uint32_t round, uint64_t idx0, size_t n, float* z) {
    g_err.clear();
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "noise: idx0 + n beyond 2^64");
    if (n == 0) return FA_OK;
    if (!z) return fail(FA_ERR_ARG, "noise: z is null");
    fa::noise_host(seed, stream, round, idx0, n, z);
    return FA_OK;
}

int fa_set_secagg(fa_ctx* ctx, int part_id, float scale) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.secagg.scale = 0.0f;
    if (scale > 0.0f || scale != scale) {  // <= 0 turns the stage off
        if (int rc = check_secagg_scale(scale)) return rc;
        if (ctx && part_id < 0)
            return fail(FA_ERR_ARG, "secagg: set on a part, not as a context default (a round's terms belong to one part)");
        c.secagg.scale = scale;
    }
    return set_stage(ctx, part_id, kSecagg, c);
}

int fa_secagg_set_terms(fa_ctx* ctx, int part_id, int T, const uint32_t* keys, const uint32_t* nonces, const int* signs) {
    g_err.clear();
    Part* p;
    if (int rc = check_part(ctx, part_id, &p)) return rc;
    if (int rc = check_secagg_terms(T, keys, nonces, signs)) return rc;
    if (!p->secagg.on()) return fail(FA_ERR_STATE, "part %d has no secagg stage", part_id);
    SecaggStage& sa = p->secagg;
    sa.tab.resize(fa::secagg_table_words(T));
    fa::secagg_table(T, keys, nonces, signs, sa.tab.data(), &sa.npos, &sa.cnet);
    sa.T = T;
    sa.have = true;
    p->ready = false;  // new terms invalidate a finished reduction, as a new receipt does
    return FA_OK;
}

// The body of fa_secagg_unmask_device; form: as launch_secagg's (the diagnostic entry forces one).
static int secagg_unmask_impl(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, uint64_t idx0, int T,
                              const uint32_t* keys, const uint32_t* nonces, const int* signs, float scale, void* d_out,
                              fa_dtype out, int form, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (D < 1) return fail(FA_ERR_ARG, "secagg: D must be >= 1");
    if (!dvalid(out)) return fail(FA_ERR_ARG, "bad dtype");
    if (int rc = check_secagg_scale(scale)) return rc;
    if (int rc = check_secagg_terms(T, keys, nonces, signs)) return rc;
    if (int rc = check_secagg_range(idx0, n)) return rc;
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if (int rc = check_clients(d_clients, D, 4, "client")) return rc;
    if (!d_out) return fail(FA_ERR_ARG, "output pointer is null");
    if (!aligned(d_out, dsize(out))) return fail(FA_ERR_ALIGN, "output not %zu-byte aligned", dsize(out));
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    std::vector<uint32_t> tab(fa::secagg_table_words(T));
    int npos = 0;
    uint32_t cnet = 0;
    fa::secagg_table(T, keys, nonces, signs, tab.data(), &npos, &cnet);
    uint32_t* d_tab = nullptr;  // a table of its own, freed before the return: the entry waits for its stream
    if (hipMalloc((void**)&d_tab, tab.size() * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FA_ERR_NOMEM, "secagg: term table alloc of %zu B failed", tab.size() * 4);
    }
    hipError_t e = hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    int rc = FA_OK;
    if (e == hipSuccess) rc = secagg_on(ctx, c.g, c.tu, d_clients, D, n, idx0, d_tab, T, npos, cnet, scale, d_out, out, form, c.s);
    const hipError_t es = hipStreamSynchronize(c.s);
    if (e == hipSuccess) e = es;
    (void)hipFree(d_tab);
    if (rc) return rc;
    FA_HIP(e);
    return FA_OK;
}

int fa_secagg_unmask_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, uint64_t idx0, int T,
                            const uint32_t* keys, const uint32_t* nonces, const int* signs, float scale, void* d_out,
                            fa_dtype out, void* hip_stream) {
    return secagg_unmask_impl(ctx, gpu, d_clients, D, n, idx0, T, keys, nonces, signs, scale, d_out, out, -1, hip_stream);
}

// Diagnostic, outside fa.h: fa_secagg_unmask_device in the vector form `form` (0 tile per wave, 1 term split)
// whatever fa_secagg_form says -- the same bits; for measuring one form against the other.
int fa_diag_secagg_unmask(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, uint64_t idx0, int T,
                          const uint32_t* keys, const uint32_t* nonces, const int* signs, float scale, void* d_out,
                          fa_dtype out, int form, void* hip_stream) {
    if (form != fa::kSecaggTile && form != fa::kSecaggSplit) {
        g_err.clear();
        return fail(FA_ERR_ARG, "secagg: form %d is neither 0 nor 1", form);
    }
    return secagg_unmask_impl(ctx, gpu, d_clients, D, n, idx0, T, keys, nonces, signs, scale, d_out, out, form, hip_stream);
}

int fa_secagg_mask_host(const uint32_t* key, const uint32_t* nonce, uint64_t idx0, size_t n, uint32_t* out) {
    g_err.clear();
    if (int rc = check_secagg_range(idx0, n)) return rc;
    if (n == 0) return FA_OK;
    if (!key || !nonce || !out) return fail(FA_ERR_ARG, "secagg: %s is null", !key ? "key" : !nonce ? "nonce" : "out");
    fa::secagg_mask_host(key, nonce, idx0, n, out);
    return FA_OK;
}

int fa_secagg_quantize(const float* v, size_t n, float q, int32_t* out, uint64_t* n_bad) {
    g_err.clear();
    if (!finite_f(q) || !(q > 0.0f)) return fail(FA_ERR_ARG, "secagg: q %g must be finite and > 0", (double)q);
    if (n_bad) *n_bad = 0;
    if (n == 0) return FA_OK;
    if (!v || !out) return fail(FA_ERR_ARG, "secagg: %s is null", !v ? "v" : "out");
    const double lim = 2147483647.0;
    uint64_t bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const double c = std::nearbyint((double)v[i] * (double)q);  // to nearest, ties to even
        if (c != c) ++bad;
        out[i] = c != c ? 0 : c > lim ? INT32_MAX : c < -lim ? -INT32_MAX : (int32_t)c;
    }
    if (n_bad) *n_bad = bad;
    return FA_OK;
}

int fa_secagg_form(size_t n, int T) { return fa::secagg_form((int64_t)n, T); }

size_t fa_sign_words(size_t n) { return n / 32 + (n % 32 ? 1 : 0); }

int fa_sign_pack(const float* delta, size_t n, uint32_t* bits) {
    g_err.clear();
    if (n == 0) return FA_OK;
    if (!delta || !bits) return fail(FA_ERR_ARG, "sign: %s is null", !delta ? "delta" : "bits");
    fa::sign_pack_host(delta, n, bits);
    return FA_OK;
}

// What fa_sign_vote_host and fa_sign_vote_device refuse before they look at a pointer's target.
static int check_sign_vote(int D, size_t n, uint64_t idx0, float eta, int rule, int margin, const void* neg, const void* pos) {
    if (int rc = check_sign_clients(D, 1)) return rc;
    if ((neg == nullptr) != (pos == nullptr)) return fail(FA_ERR_ARG, "sign: %s plane without the other", neg ? "the neg" : "the pos");
    if (int rc = check_sign_params(eta, rule, margin, false)) return rc;
    if (neg && rule == FA_SIGN_MEAN) return fail(FA_ERR_ARG, "sign: the vote planes exist under the majority rule only");
    if (int rc = check_sign_clients(D, margin)) return rc;
    if (idx0 % 32) return fail(FA_ERR_ARG, "sign: idx0 %llu is no multiple of 32", (unsigned long long)idx0);
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "sign: idx0 + n beyond 2^64");
    return FA_OK;
}

int fa_sign_vote_host(const uint32_t* const* bits, int D, size_t n, uint64_t idx0, float eta, int rule, int margin,
                      const float* ref, float* out, uint32_t* neg, uint32_t* pos) {
    g_err.clear();
    if (int rc = check_sign_vote(D, n, idx0, eta, rule, margin, neg, pos)) return rc;
    if (n == 0) return FA_OK;
    if (int rc = check_clients(reinterpret_cast<const void* const*>(bits), D, 4, "receipt")) return rc;
    if (!out) return fail(FA_ERR_ARG, "sign: out is null");
    fa::sign_vote_host(bits, D, n, idx0, eta, rule, margin, ref, out, neg, pos);
    return FA_OK;
}

// The receipts at the word of idx0 (into at), after the checks of the pointers fa_sign_vote_device and fa_sign_form share.
static int sign_operands(const uint32_t* const* d_bits, int D, uint64_t idx0, const void* d_ref, fa_dtype rdt, const void* d_out,
                         fa_dtype odt, const void* d_neg, const void* d_pos, std::vector<const uint32_t*>* at) {
    if (int rc = check_clients(reinterpret_cast<const void* const*>(d_bits), D, 4, "receipt")) return rc;
    if (!d_out) return fail(FA_ERR_ARG, "output pointer is null");
    if (d_ref && !aligned(d_ref, dsize(rdt))) return fail(FA_ERR_ALIGN, "sign: reference not %zu-byte aligned", dsize(rdt));
    if (!aligned(d_out, dsize(odt))) return fail(FA_ERR_ALIGN, "output not %zu-byte aligned", dsize(odt));
    if (d_neg && (!aligned(d_neg, 4) || !aligned(d_pos, 4))) return fail(FA_ERR_ALIGN, "sign: planes not 4-byte aligned");
    at->resize((size_t)D);
    for (int k = 0; k < D; ++k) (*at)[(size_t)k] = d_bits[k] + (idx0 >> 5);
    return FA_OK;
}

int fa_sign_vote_device(fa_ctx* ctx, int gpu, const uint32_t* const* d_bits, int D, size_t n, uint64_t idx0, float eta,
                        int rule, int margin, const void* d_ref, fa_dtype ref_dtype, void* d_out, fa_dtype out_dtype,
                        uint32_t* d_neg, uint32_t* d_pos, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!dvalid(out_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    FA_PAIR(ref_dtype, out_dtype);
    if (int rc = check_sign_vote(D, n, idx0, eta, rule, margin, d_neg, d_pos)) return rc;
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    std::vector<const uint32_t*> at;
    if (int rc = sign_operands(d_bits, D, idx0, d_ref, ref_dtype, d_out, out_dtype, d_neg, d_pos, &at)) return rc;
    if (d_ref) {
        const uintptr_t o = (uintptr_t)d_out, r = (uintptr_t)d_ref;
        if (o < r + n * dsize(ref_dtype) && r < o + n * dsize(out_dtype)) return fail(FA_ERR_ARG, "sign: d_out overlaps d_ref");
    }
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    SignCfg cfg;
    cfg.eta = eta;
    cfg.rule = rule;
    cfg.margin = margin;
    return sign_on(c.tu, at.data(), D, n, cfg, d_ref, ref_dtype, d_out, out_dtype, d_neg, d_pos, c.s);
}

int fa_sign_form(size_t n, const uint32_t* const* d_bits, int D, uint64_t idx0, const void* d_ref, fa_dtype ref_dtype,
                 const void* d_out, fa_dtype out_dtype, const void* d_neg, const void* d_pos) {
    g_err.clear();
    if (!dvalid(out_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (int rc = check_sign_clients(D, 1)) return rc;
    if (idx0 % 32) return fail(FA_ERR_ARG, "sign: idx0 %llu is no multiple of 32", (unsigned long long)idx0);
    std::vector<const uint32_t*> at;
    if (int rc = sign_operands(d_bits, D, idx0, d_ref, ref_dtype, d_out, out_dtype, d_neg, d_pos, &at)) return rc;
    return fa::sign_split(at.data(), D, n, d_ref, ref_dtype, d_out, out_dtype, d_neg, d_pos).vec ? 1 : 0;
}

int fa_set_sign(fa_ctx* ctx, int part_id, float eta, int rule, int margin, int planes) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.sign = SignCfg{};
    if (eta > 0.0f || eta != eta) {  // <= 0 turns the stage off
        if (int rc = check_sign_params(eta, rule, margin, planes != 0)) return rc;
        if (ctx && part_id < 0)
            return fail(FA_ERR_ARG, "sign: set on a part, not as a context default (a round's receipts belong to one part)");
        c.sign.eta = eta;
        c.sign.rule = rule;
        c.sign.margin = margin;
        c.sign.planes = planes != 0;
    }
    return set_stage(ctx, part_id, kSign, c);
}

int fa_submit_sign(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* bits, int flags) {
    g_err.clear();
    return submit_sign_impl(ctx, part_id, client_slot, bits, flags);
}

int fa_copy_sign_planes(fa_ctx* ctx, int part_id, uint32_t* neg, uint32_t* pos) {
    g_err.clear();
    Part* p;
    if (int rc = check_part(ctx, part_id, &p)) return rc;
    if (!p->sign.on() || !p->sign.has_planes || !p->sign.planes)
        return fail(FA_ERR_STATE, "sign: part %d has no vote planes (%s)", part_id,
                    !p->sign.on() ? "no sign-vote stage" : "fa_set_sign without planes, or no reducing call since");
    if (p->n && (!neg || !pos)) return fail(FA_ERR_ARG, "sign: %s is null", !neg ? "neg" : "pos");
    for (int g = 0; g < ctx->G; ++g) {  // ordered after the reducing call as copy_output is
        GpuRes& r = ctx->gpu[(size_t)g];
        const size_t cnt = p->cnt[(size_t)g], w0 = p->off[(size_t)g] >> 5, bytes = sign_words(cnt) * 4;
        if (!cnt) continue;
        DeviceGuard dg(r.dev);
        hipStream_t ds = p->done_stream[(size_t)g];
        if (ds && ds != r.compute) {
            FA_HIP(hipEventRecord(p->done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.compute, p->done[(size_t)g], 0));
        }
        const char* src = p->sign.planes.at((size_t)g);
        FA_HIP(hipMemcpyAsync(neg + w0, src, bytes, hipMemcpyDeviceToHost, r.compute));
        FA_HIP(hipMemcpyAsync(pos + w0, src + p->sign.stride[(size_t)g], bytes, hipMemcpyDeviceToHost, r.compute));
    }
    for (int g = 0; g < ctx->G; ++g) {
        DeviceGuard dg(ctx->gpu[(size_t)g].dev);
        FA_HIP(hipStreamSynchronize(ctx->gpu[(size_t)g].compute));
    }
    return FA_OK;
}

int fa_set_sparse_sum(fa_ctx* ctx, int part_id, size_t k_max) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.sparse = SparseCfg{};
    if (k_max) {  // 0 turns the stage off
        if (ctx && part_id < 0)
            return fail(FA_ERR_ARG, "sparse: set on a part, not as a context default (a round's receipts belong to one part)");
        c.sparse.k_max = k_max;
    }
    return set_stage(ctx, part_id, kSparse, c);
}

int fa_submit_sparse(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* idx, const float* val, size_t k, float weight,
                     int flags) {
    g_err.clear();
    return submit_sparse_impl(ctx, part_id, client_slot, idx, val, k, weight, flags);
}

int fa_set_mx8_sum(fa_ctx* ctx, int part_id, int on) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.mx8sum = Mx8SumCfg{};
    if (on) {
        if (ctx && part_id < 0)
            return fail(FA_ERR_ARG, "mx8 sum: set on a part, not as a context default (a round's receipts belong to one part)");
        c.mx8sum.flag = true;
    }
    return set_stage(ctx, part_id, kMx8Sum, c);
}

int fa_submit_mx8_sum(fa_ctx* ctx, int part_id, int client_slot, const int8_t* q, const uint8_t* e, float weight, int flags) {
    g_err.clear();
    return submit_mx8_sum_impl(ctx, part_id, client_slot, q, e, weight, flags);
}

int fa_set_lowrank_sum(fa_ctx* ctx, int part_id, const fa_lowrank_mat* mats, size_t M, int r_max) {
    g_err.clear();
    if (!ctx) return fail(FA_ERR_ARG, "ctx is null");
    if (part_id < 0)
        return fail(FA_ERR_ARG, "lowrank sum: set on a part, not as a context default (a table belongs to one part's layout)");
    StageCfgs c = requested(ctx);
    c.lrsum = LowrankSumCfg{};
    if (M) {
        Part* p;
        if (int rc = check_part(ctx, part_id, &p)) return rc;
        if (int rc = fa_lowrank_check(mats, M, p->n)) return rc;
        if (r_max < 1 || r_max > FA_LOWRANK_MAX_RANK)
            return fail(FA_ERR_ARG, "lowrank sum: r_max %d outside 1 .. %d", r_max, FA_LOWRANK_MAX_RANK);
        c.lrsum.mats.assign(mats, mats + M);
        c.lrsum.r_max = r_max;
    }
    return set_stage(ctx, part_id, kLowrankSum, c);
}

int fa_submit_lowrank_sum(fa_ctx* ctx, int part_id, int client_slot, const float* f, size_t len, int r, float weight,
                          int flags) {
    g_err.clear();
    return submit_lowrank_sum_impl(ctx, part_id, client_slot, f, len, r, weight, flags);
}

int fa_set_rot1_sum(fa_ctx* ctx, int part_id, int on) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.rot1sum = Rot1SumCfg{};
    if (on) {
        if (ctx && part_id < 0)
            return fail(FA_ERR_ARG, "rot1 sum: set on a part, not as a context default (a round's receipts belong to one part)");
        c.rot1sum.flag = true;
    }
    return set_stage(ctx, part_id, kRot1Sum, c);
}

int fa_submit_rot1_sum(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* bits, const float* scale, uint64_t seed,
                       float weight, int flags) {
    g_err.clear();
    return submit_rot1_sum_impl(ctx, part_id, client_slot, bits, scale, seed, weight, flags);
}

size_t fa_mx8_scale_bytes(size_t n) { return n / FA_MX8_BLOCK + (n % FA_MX8_BLOCK ? 1 : 0); }

int fa_mx8_encode(const float* delta, size_t n, int8_t* q, uint8_t* e) {
    g_err.clear();
    if (n == 0) return FA_OK;
    if (!delta || !q || !e) return fail(FA_ERR_ARG, "mx8: %s is null", !delta ? "delta" : !q ? "q" : "e");
    fa::mx8_encode_host(delta, n, q, e);
    return FA_OK;
}

int fa_mx8_decode(const int8_t* q, const uint8_t* e, size_t n, uint64_t idx0, float* d) {
    g_err.clear();
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "mx8: idx0 + n beyond 2^64");
    if (n == 0) return FA_OK;
    if (!q || !e || !d) return fail(FA_ERR_ARG, "mx8: %s is null", !q ? "q" : !e ? "e" : "d");
    fa::mx8_decode_host(q, e, n, idx0, d);
    return FA_OK;
}

int fa_mx8_expand_device(fa_ctx* ctx, int gpu, const int8_t* d_q, const uint8_t* d_e, size_t n, uint64_t idx0,
                         const void* d_ref, fa_dtype ref_dtype, void* d_dst, fa_dtype dst_dtype, void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!dvalid(dst_dtype) || !dvalid(ref_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (!fa::dtype_pair_ok(dst_dtype, ref_dtype))
        return fail(FA_ERR_ARG, "mx8: no %s slot against a %s reference (a 16-bit slot takes its own type or f32)",
                    fa::dtype_name(dst_dtype), fa::dtype_name(ref_dtype));
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "mx8: idx0 + n beyond 2^64");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    if (!d_q || !d_e || !d_dst) return fail(FA_ERR_ARG, "mx8: %s pointer is null", !d_q ? "d_q" : !d_e ? "d_e" : "d_dst");
    if (d_ref && !aligned(d_ref, dsize(ref_dtype)))
        return fail(FA_ERR_ALIGN, "mx8: reference not %zu-byte aligned", dsize(ref_dtype));
    if (!aligned(d_dst, dsize(dst_dtype))) return fail(FA_ERR_ALIGN, "mx8: slot not %zu-byte aligned", dsize(dst_dtype));
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    FA_HIP(fa::launch_mx8_expand(d_q, d_e, idx0, (int64_t)n, d_ref, ref_dtype, d_dst, dst_dtype, c.s));
    return FA_OK;
}

int fa_set_mx8(fa_ctx* ctx, int part_id, int on) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.mx8 = receipts_of(ctx, part_id);
    c.mx8.flag = on != 0;
    return set_stage(ctx, part_id, kMx8, c);
}

int fa_set_topk(fa_ctx* ctx, int part_id, size_t k_max) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.mx8 = receipts_of(ctx, part_id);
    c.mx8.k_max = k_max;
    return set_stage(ctx, part_id, kMx8, c);
}

int fa_submit_topk(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* idx, const float* val, size_t k, float weight,
                   int flags) {
    g_err.clear();
    return submit_topk_impl(ctx, part_id, client_slot, idx, val, k, weight, flags);
}

int fa_set_lowrank(fa_ctx* ctx, int part_id, const fa_lowrank_mat* mats, size_t M, int r_max) {
    g_err.clear();
    if (!ctx) return fail(FA_ERR_ARG, "ctx is null");
    if (part_id < 0) return fail(FA_ERR_ARG, "lowrank: a table belongs to one part's layout: there is no context default");
    StageCfgs c = requested(ctx);
    c.mx8 = receipts_of(ctx, part_id);
    c.mx8.mats.clear();
    c.mx8.r_max = 0;
    if (M) {
        Part* p;
        if (int rc = check_part(ctx, part_id, &p)) return rc;
        if (int rc = fa_lowrank_check(mats, M, p->n)) return rc;
        if (r_max < 1 || r_max > FA_LOWRANK_MAX_RANK)
            return fail(FA_ERR_ARG, "lowrank: r_max %d outside 1 .. %d", r_max, FA_LOWRANK_MAX_RANK);
        c.mx8.mats.assign(mats, mats + M);
        c.mx8.r_max = r_max;
    }
    return set_stage(ctx, part_id, kMx8, c);
}

int fa_submit_lowrank(fa_ctx* ctx, int part_id, int client_slot, const float* f, size_t len, int r, float weight, int flags) {
    g_err.clear();
    return submit_lowrank_impl(ctx, part_id, client_slot, f, len, r, weight, flags);
}

int fa_set_rot1(fa_ctx* ctx, int part_id, int on) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.mx8 = receipts_of(ctx, part_id);
    c.mx8.rot1 = on != 0;
    return set_stage(ctx, part_id, kMx8, c);
}

int fa_submit_rot1(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* bits, const float* scale, uint64_t seed,
                   float weight, int flags) {
    g_err.clear();
    return submit_rot1_impl(ctx, part_id, client_slot, bits, scale, seed, weight, flags);
}

int fa_submit_mx8(fa_ctx* ctx, int part_id, int client_slot, const int8_t* q, const uint8_t* e, float weight, int flags) {
    g_err.clear();
    return submit_mx8_impl(ctx, part_id, client_slot, q, e, weight, flags);
}

int fa_mx8_set_reference(fa_ctx* ctx, int part_id, const void* host_src) {
    g_err.clear();
    Part* p;
    if (int rc = check_part(ctx, part_id, &p)) return rc;
    if (!p->mx8.on() && !p->reply.on() && !p->sign.on() && !p->sparse.on() && !p->mx8sum.on() && !p->lrsum.on() && !p->rot1sum.on())
        return fail(FA_ERR_STATE, "mx8: part %d neither takes MX8 receipts (fa_set_mx8) nor sends MX8 replies "
                                  "(fa_set_mx8_reply), nor takes top-k (fa_set_topk), low-rank (fa_set_lowrank) or rot1 receipts (fa_set_rot1), "
                                  "nor has a sign-vote (fa_set_sign), sparse-sum (fa_set_sparse_sum), MX8-sum (fa_set_mx8_sum), low-rank-sum (fa_set_lowrank_sum) or rot1-sum stage (fa_set_rot1_sum)", part_id);
    if (!host_src && p->n) return fail(FA_ERR_ARG, "mx8: host_src is null");
    if (int rc = wait_devices(ctx)) return rc;  // the part's pending work, on whatever stream
    if (p->reply.on())
        if (int rc = ensure_reply_buf(ctx, *p)) return rc;
    const size_t so = dsize(p->out);
    for (int g = 0; g < ctx->G; ++g) {
        DeviceGuard dg(ctx->gpu[(size_t)g].dev);
        if (!p->cnt[(size_t)g]) continue;
        const char* src = static_cast<const char*>(host_src) + p->off[(size_t)g] * so;
        FA_HIP(hipMemcpy(p->dout[(size_t)g], src, p->cnt[(size_t)g] * so, hipMemcpyHostToDevice));
        if (p->reply.on())  // the owners hold it: the next reply is taken against it
            FA_HIP(hipMemcpy(p->reply.sent.at((size_t)g), src, p->cnt[(size_t)g] * so, hipMemcpyHostToDevice));
    }
    if (p->reply.on()) p->reply.has_sent = true;
    set_range_runs(*p, ctx->G);  // as a round's output: the reference, and what fa_copy_output hands out
    return FA_OK;
}

int fa_mx8_encode_device(fa_ctx* ctx, int gpu, const void* d_new, fa_dtype new_dtype, const void* d_sent,
                         fa_dtype sent_dtype, size_t n, uint64_t idx0, int8_t* d_q, uint8_t* d_e, void* d_out, int flags,
                         void* hip_stream) {
    g_err.clear();
    // every check before any device call: with n == 0 this is the feature probe of a box without a GPU
    if (!dvalid(new_dtype) || !dvalid(sent_dtype)) return fail(FA_ERR_ARG, "bad dtype");
    if (new_dtype != sent_dtype)
        return fail(FA_ERR_ARG, "mx8 reply: the new model is %s, the sent one %s: one dtype", fa::dtype_name(new_dtype),
                    fa::dtype_name(sent_dtype));
    if (flags & ~(FA_MX8_SCALES_ONLY | FA_MX8_SCALES_GIVEN)) return fail(FA_ERR_ARG, "mx8 reply: unknown flags 0x%x", flags);
    if ((flags & FA_MX8_SCALES_ONLY) && (flags & FA_MX8_SCALES_GIVEN))
        return fail(FA_ERR_ARG, "mx8 reply: FA_MX8_SCALES_ONLY and FA_MX8_SCALES_GIVEN exclude each other");
    if (idx0 + (uint64_t)n < idx0) return fail(FA_ERR_ARG, "mx8 reply: idx0 + n beyond 2^64");
    if (ctx && (gpu < 0 || gpu >= ctx->G)) return fail(FA_ERR_ARG, "gpu %d out of range", gpu);
    if (n == 0) return FA_OK;
    const bool only = (flags & FA_MX8_SCALES_ONLY) != 0;
    if (!d_new || !d_sent || !d_e || (!only && !d_q))
        return fail(FA_ERR_ARG, "mx8 reply: %s pointer is null", !d_new ? "d_new" : !d_sent ? "d_sent" : !d_e ? "d_e" : "d_q");
    const size_t es = dsize(new_dtype);
    if (!aligned(d_new, es) || !aligned(d_sent, es) || (!only && d_out && !aligned(d_out, es)))
        return fail(FA_ERR_ALIGN, "mx8 reply: %s not %zu-byte aligned", !aligned(d_new, es) ? "d_new" : !aligned(d_sent, es) ? "d_sent" : "d_out", es);
    if (!only && d_out) {  // the same address as an input, or apart from it
        const uintptr_t o = (uintptr_t)d_out, bytes = (uintptr_t)(n * es);
        for (const void* in : {d_new, d_sent}) {
            const uintptr_t a = (uintptr_t)in;
            if (o != a && o < a + bytes && a < o + bytes)
                return fail(FA_ERR_ARG, "mx8 reply: d_out overlaps %s without being it", in == d_new ? "d_new" : "d_sent");
        }
    }
    const DeviceCall c = device_call(ctx, gpu, hip_stream);
    DeviceGuard dg(c.dev);
    const int mode = only ? fa::kMx8EncScalesOnly : (flags & FA_MX8_SCALES_GIVEN) ? fa::kMx8EncScalesGiven : fa::kMx8EncFused;
    FA_HIP(fa::launch_mx8_encode(d_new, d_sent, new_dtype, idx0, (int64_t)n, d_q, d_e, only ? nullptr : d_out, nullptr, mode,
                                 c.s));
    return FA_OK;
}

int fa_set_mx8_reply(fa_ctx* ctx, int part_id, int on) {
    g_err.clear();
    StageCfgs c = requested(ctx);
    c.reply.flag = on != 0;
    return set_stage(ctx, part_id, kReply, c);
}

namespace {

// D2H of the codes of the part's last reducing call, ordered after it as copy_output is; counts the E = 255 blocks
// on the way.  A block's scale byte lies in one GPU's range (reply_stage), so the copies do not overlap.
int copy_mx8_codes(fa_ctx* ctx, Part& p, int8_t* q, uint8_t* e) {
    const int G = ctx->G;
    for (int g = 0; g < G; ++g) {
        GpuRes& r = ctx->gpu[(size_t)g];
        const size_t cnt = p.cnt[(size_t)g], off = p.off[(size_t)g];
        if (!cnt) continue;
        DeviceGuard dg(r.dev);
        hipStream_t ds = p.done_stream[(size_t)g];
        if (ds && ds != r.compute) {
            FA_HIP(hipEventRecord(p.done[(size_t)g], ds));
            FA_HIP(hipStreamWaitEvent(r.compute, p.done[(size_t)g], 0));
        }
        const char* src = p.reply.codes.at((size_t)g);
        if (q) FA_HIP(hipMemcpyAsync(q + off, src, cnt, hipMemcpyDeviceToHost, r.compute));
        FA_HIP(hipMemcpyAsync(e + (off >> 5), src + p.reply.eoff[(size_t)g], ((off + cnt - 1) >> 5) - (off >> 5) + 1,
                              hipMemcpyDeviceToHost, r.compute));
    }
    for (int g = 0; g < G; ++g) {
        DeviceGuard dg(ctx->gpu[(size_t)g].dev);
        FA_HIP(hipStreamSynchronize(ctx->gpu[(size_t)g].compute));
    }
    uint64_t nan = 0;
    for (size_t b = 0, B = fa_mx8_scale_bytes(p.n); b < B; ++b) nan += e[b] == 255;
    p.reply.nan = nan;
    p.reply.counted = true;
    return FA_OK;
}

int check_mx8_dst(const Part& p, const void* q, const void* e, int flags) {
    if (flags & ~FA_HOST_PINNED) return fail(FA_ERR_ARG, "unknown flags 0x%x", flags);
    if (p.n && (!q || !e)) return fail(FA_ERR_ARG, "mx8 reply: %s is null", !q ? "q" : "e");
    return FA_OK;
}

}  // namespace

int fa_finalize_mx8(fa_ctx* ctx, int part_id, int8_t* q, uint8_t* e, int flags) {
    g_err.clear();
    Trace tr("fa_finalize_mx8 part %d", part_id);
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc || (rc = check_mx8_dst(*p, q, e, flags))) return rc;
    // the round as it stands decides, before any work: reduced already, it has codes or not; else it will have
    // them if the owners hold a model
    if (!p->reply.on() || (p->ready ? !p->reply.has_codes : !p->reply.has_sent))
        return fail(FA_ERR_STATE, "mx8 reply: part %d has %s: finish the round with fa_finalize", part_id,
                    !p->reply.on() ? "no reply stage (fa_set_mx8_reply)" : "no sent model yet (the bootstrap round)");
    if (p->n_submitted != p->D)
        return fail(FA_ERR_STATE, "part %d: %d of %d clients submitted", part_id, p->n_submitted, p->D);
    if (!p->ready && (rc = reduce_part(ctx, *p, p->w.data(), nullptr))) return rc;
    if (p->n && (rc = copy_mx8_codes(ctx, *p, q, e))) return rc;
    reset_round(*p);
    return FA_OK;
}

int fa_copy_mx8(fa_ctx* ctx, int part_id, int8_t* q, uint8_t* e, int flags) {
    g_err.clear();
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc || (rc = check_mx8_dst(*p, q, e, flags))) return rc;
    if (!p->reply.on() || !p->reply.has_codes)
        return fail(FA_ERR_STATE, "mx8 reply: part %d has no codes (%s)", part_id,
                    !p->reply.on() ? "no reply stage" : "no reducing call yet, or the last one was the bootstrap");
    return p->n ? copy_mx8_codes(ctx, *p, q, e) : FA_OK;
}

int fa_mx8_reply_stats(fa_ctx* ctx, int part_id, uint64_t* nan_blocks) {
    g_err.clear();
    Part* p;
    int rc = check_part(ctx, part_id, &p);
    if (rc) return rc;
    if (!p->reply.on()) return fail(FA_ERR_STATE, "mx8 reply: part %d has no reply stage (fa_set_mx8_reply)", part_id);
    if (!p->reply.counted && p->n) {  // nobody fetched the codes yet: the scale bytes alone
        std::vector<uint8_t> e(fa_mx8_scale_bytes(p->n));
        if ((rc = copy_mx8_codes(ctx, *p, nullptr, e.data()))) return rc;
    }
    if (nan_blocks) *nan_blocks = p->reply.nan;
    return FA_OK;
}

}  // extern "C"
