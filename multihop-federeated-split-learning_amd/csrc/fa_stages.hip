// fa_stages.hip -- the aggregation stages of libfa (fa.h: server optimizer, clip, Krum, geomed, Bulyan, noise, MX8
// receipts, MX8 replies) and their entries of the C ABI.  A stage is one struct (fa_host.h), one row of the admission
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
    p.mx8 = Mx8Stage{};
}
void free_reply(fa_ctx* ctx, Part& p) {
    for (DevArrays* a : {&p.reply.sent, &p.reply.codes}) a->free(ctx->gpu);
    p.reply = ReplyStage{};
}
void free_stages(fa_ctx* ctx, Part& p) {
    p.noise = NoiseStage{};
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
    // Krum, geomed (never with each other or with clip) and Bulyan (an FA_TRIMMED part: never with those three): the
    // passes, the host's waits for their results, and the selection or the new weights
    if (p.krum.on() || p.geomed.on()) rd->subset = true;
    if (p.krum.on()) return krum_plan(ctx, p, w, s, &rd->plan);
    if (p.geomed.on()) return geomed_plan(ctx, p, w, s, &rd->plan);
    if (p.bulyan.on()) return bulyan_plan(ctx, p, s, &rd->plan);
    return FA_OK;
}

// The aggregate into adst (dst without a server optimizer or a noise stage; with one in fp32 -- an f32 part: in its
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

// fa_set_mx8 / fa_set_mx8_reply on a part (not FA_LITERAL, not rs).  Off: what the stage allocated goes, after the
// devices' pending work.  On, for a part without it: what this round kept host-side or chained so far goes back to the
// plain path; the buffers come with the first fa_submit_mx8, or the first reducing call.
int set_part_flag(fa_ctx* ctx, Part& p, bool reply, bool on) {
    const bool was = reply ? p.reply.on() : p.mx8.on();
    if (on == was) return FA_OK;
    if (int rc = on ? host_flush(ctx, p) : wait_devices(ctx)) return rc;
    if (!on) {
        reply ? free_reply(ctx, p) : free_mx8(ctx, p);
        return FA_OK;
    }
    restart_round_plain(p);
    (reply ? p.reply.cfg : p.mx8.cfg).flag = true;
    return FA_OK;
}

int set_part_stage(fa_ctx* ctx, Part& p, StageId id, const StageCfgs& c) {
    switch (id) {
        case kOpt: return set_part_opt(ctx, p, c.opt);
        case kClip: return set_part_clip(ctx, p, c.clip);
        case kKrum: return set_part_select(p, p.krum, c.krum);
        case kGeomed: return set_part_select(p, p.geomed, c.geomed);
        case kBulyan: return set_part_bulyan(p, c.bulyan);
        case kNoise: return set_part_noise(ctx, p, c.noise);
        default: return set_part_flag(ctx, p, id == kReply, id == kReply ? c.reply.flag : c.mx8.flag);
    }
}

// ------------------------------------------------------------------ the admission rule

// One row per stage, in StageId order: its name as the refusals begin, its name as in "has a Krum stage", the bucket
// modes it applies to (a bit per fa_mode), whether it belongs to the measure-then-select family (at most one per part,
// and at most one among the context defaults), and the tails of its refusals of an rs context and of a part's mode.
struct StageRule {
    const char *name, *title;
    unsigned modes;
    bool family;
    const char *rs_tail, *mode_tail;
};
constexpr unsigned kAvg = 1u << FA_FEDAVG, kTrim = 1u << FA_TRIMMED;
const StageRule kRules[kStages] = {
    {"server opt", "server-optimizer", kAvg | kTrim, false, "its aggregate is not bit-specified", ""},
    {"clip", "clip", kAvg, true, "its aggregate is not bit-specified; use FA_SHARD_RANGE", " (the stage clips FA_FEDAVG updates)"},
    {"krum", "Krum", kAvg, true, "a pair's distance needs both clients on one GPU; use FA_SHARD_RANGE",
     " (the stage selects the owners of an FA_FEDAVG average)"},
    {"geomed", "geomed", kAvg, true, "a distance needs every client of an element on one GPU; use FA_SHARD_RANGE",
     " (the stage re-weights the owners of an FA_FEDAVG average)"},
    {"bulyan", "Bulyan", kTrim, false, "the rule needs every client on one GPU; use FA_SHARD_RANGE",
     " (the stage replaces the window of an FA_TRIMMED part)"},
    {"noise", "noise", kAvg | kTrim, false, "its aggregate is not bit-specified; use FA_SHARD_RANGE", ""},
    {"mx8", "MX8", kAvg | kTrim, false, "a GPU holding a whole slot does not hold the matching output; use FA_SHARD_RANGE", ""},
    {"mx8 reply", "reply", kAvg | kTrim, false, "use FA_SHARD_RANGE", ""},
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
    return FA_OK;
}

// The check of a stage's numbers against a part's D clients, for the stages that have one (Krum's m = -1 is resolved).
int check_for_clients(StageId id, int D, StageCfgs& c) {
    if (id == kKrum) return check_krum(D, c.krum.f, c.krum.m, &c.krum.m);
    if (id == kGeomed) return check_geomed(D, c.geomed.iters, c.geomed.nu);
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
    if (report && !(id == kClip ? p.clip.reported : id == kKrum ? p.krum.reported : id == kGeomed ? p.geomed.reported : p.bulyan.reported))
        return fail(FA_ERR_STATE, "part %d: no round reduced with the %s stage yet", part_id, kRules[id].title);
    return FA_OK;
}

// ------------------------------------------------------------------ MX8 receipts (fa.h "MX8 receipts")

// The scale bytes GPU g's range [off, off + cnt) touches: blocks off >> 5 .. (off + cnt - 1) >> 5.
inline size_t mx8_scales(size_t off, size_t cnt) { return cnt ? ((off + cnt - 1) >> 5) - (off >> 5) + 1 : 0; }

// The shadows of an MX8 part, allocated once: per GPU held x stride bytes.  q lies at the shadow's start, which
// keeps the 16-byte phase of the slots and the output (all 16-byte aligned: the vector form applies).  On failure the
// part stays an MX8 part.
int ensure_mx8_buf(fa_ctx* ctx, Part& p) {
    Mx8Stage& s = p.mx8;
    if (s.buf) return FA_OK;
    s.stride.clear();
    s.eoff.clear();
    for (size_t g = 0; g < (size_t)ctx->G; ++g) {
        s.eoff.push_back((p.cnt[g] + 15) / 16 * 16);
        s.stride.push_back((s.eoff[g] + mx8_scales(p.off[g], p.cnt[g]) + 255) / 256 * 256);
    }
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
    if (!p->mx8.on()) return fail(FA_ERR_STATE, "mx8: part %d does not take MX8 receipts (fa_set_mx8)", part_id);
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
    c.mx8.flag = on != 0;
    return set_stage(ctx, part_id, kMx8, c);
}

int fa_submit_mx8(fa_ctx* ctx, int part_id, int client_slot, const int8_t* q, const uint8_t* e, float weight, int flags) {
    g_err.clear();
    return submit_mx8_impl(ctx, part_id, client_slot, q, e, weight, flags);
}

int fa_mx8_set_reference(fa_ctx* ctx, int part_id, const void* host_src) {
    g_err.clear();
    Part* p;
    if (int rc = check_part(ctx, part_id, &p)) return rc;
    if (!p->mx8.on() && !p->reply.on())
        return fail(FA_ERR_STATE, "mx8: part %d neither takes MX8 receipts (fa_set_mx8) nor sends MX8 replies "
                                  "(fa_set_mx8_reply)", part_id);
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
