// fa_host.h -- what libfa's two host translation units share: fa_api.hip (contexts, layouts, submits, the skeleton of
// the reduction, finalize, diagnostics) and fa_stages.hip (the aggregation stages).  Internal: the ABI is fa.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fa_internal.h"

namespace fah {

extern thread_local std::string g_err;  // fa_last_error

constexpr size_t kSkewAuto = SIZE_MAX;  // fa_tuning.slot_skew -2: chosen per bucket by slot_skew_for

// Per-context tuning (fa_ctx_set_tuning); fa_set_tuning sets the process defaults that new contexts and
// context-less fa_reduce_device calls start from.
struct CtxTuning {
    // block 128, one-shot grid, 16 clients per load group, nt loads, write-through (sc1) stores, phased
    // walk with the larger register stage where a bucket holds a phase (tools/sweep.py over 3
    // pools, profiles/r01_summary.json: sc1 stores 2.7% faster than nt, unroll 16 ~1% faster than 8,
    // block 128 2-3% faster than 256; the phased walk 1.269 ms on the north star in every pool).
    fa::Tuning tu{128, 0, 16, 1, 2, 4};
    // Byte skew between consecutive client slots of one bucket (see slot_stride); kSkewAuto = by slot size.
    size_t slot_skew = kSkewAuto;
    // FA_SHARD_CLIENT_RS: pieces per round (the reduce-scatter of piece c overlaps the reduce of c+1).
    int rs_chunks = 8;
    // Range pieces (piece_len_for): bytes of slots per piece (0 = never cut) and the span of a GPU's slots
    // above which they are cut.
    size_t piece_span = size_t(16) << 30;
    size_t piece_split = size_t(48) << 30;
};

// A roctx range around a host-side entry (submit, finalize, batched reduce, ...), so that
// `rocprofv3 --marker-trace` shows the aggregation round's host phases beside its kernels and copies.
struct Trace {
    explicit Trace(const char* fmt, int a = -1, int b = -1) {
        char buf[96];
        snprintf(buf, sizeof buf, fmt, a, b);
        roctxRangePushA(buf);
    }
    ~Trace() { roctxRangePop(); }
};

int fail(int code, const char* fmt, ...);  // sets fa_last_error, returns code

#define FA_HIP(call)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return fail(FA_ERR_HIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                     \
    } while (0)

#define FA_NCCL(call)                                                                                   \
    do {                                                                                                \
        ncclResult_t r_ = (call);                                                                       \
        if (r_ != ncclSuccess) return fail(FA_ERR_NCCL, "%s: %s (%s:%d)", #call, ncclGetErrorString(r_), \
                                           __FILE__, __LINE__);                                         \
    } while (0)

inline size_t dsize(fa_dtype t) { return t == FA_F32 ? 4 : 2; }
inline bool dvalid(int t) { return t == FA_F32 || t == FA_BF16 || t == FA_F16; }
// The refusal of a dtype pair the kernels do not have (fa::dtype_pair_ok): bf16 <-> f16.
#define FA_PAIR(in, out)                                                                                    \
    do {                                                                                                    \
        if (!fa::dtype_pair_ok((fa_dtype)(in), (fa_dtype)(out)))                                            \
            return fail(FA_ERR_ARG, "no %s -> %s reduction (a 16-bit bucket keeps its type or goes through f32)", \
                        fa::dtype_name((fa_dtype)(in)), fa::dtype_name((fa_dtype)(out)));                   \
    } while (0)

// Restores the caller's current device on scope exit.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (dev >= 0 && dev != prev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

constexpr size_t kStageBytes = 32u << 20;  // pinned staging chunk per buffer
constexpr int kSegRing = 4;                // device segment tables per GPU (GpuRes::seg)

// Host memcpy into / out of the pinned staging chunks, split over worker threads:
// one thread copies ~8-10 GB/s, a PCIe Gen5 x16 link takes ~50 GB/s.  One pool per GPU, so the GPUs of a
// range-sharded context stage their pieces concurrently.
class CopyPool {
public:
    explicit CopyPool(int n) : n_(std::max(1, n)) {
        for (int i = 1; i < n_; ++i) th_.emplace_back([this, i] { loop(i); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
            ++gen_;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    int size() const { return n_; }
    // fn(i) for every i in [0, size()): i = 0 on the calling thread, the others on the workers; returns when
    // all have.  One caller at a time.
    void run(const std::function<void(int)>& fn) {
        if (n_ == 1) {
            fn(0);
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = &fn;
            pending_ = n_ - 1;
            ++gen_;
        }
        cv_.notify_all();
        fn(0);
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [&] { return pending_ == 0; });
    }
    // dst[0, len) = src(0, len), split over the workers (the caller copies part 0).
    void copy(char* dst, size_t len, const std::function<void(size_t, size_t, char*)>& src) {
        if (n_ == 1 || len < (4u << 20)) {
            src(0, len, dst);
            return;
        }
        const size_t per = (len / n_ + 4095) / 4096 * 4096;
        run([&](int p) {
            const size_t lo = std::min(len, (size_t)p * per), hi = std::min(len, lo + per);
            if (hi > lo) src(lo, hi - lo, dst + lo);
        });
    }

private:
    void loop(int id) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)>* job;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                job = job_;
            }
            (*job)(id);
            {
                std::lock_guard<std::mutex> g(m_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    int n_;
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    uint64_t gen_ = 0;
    int pending_ = 0;
    bool stop_ = false;
    const std::function<void(int)>* job_ = nullptr;
};

// Runs fn(g) for g in [0, G): G > 1 on the context's persistent per-GPU workers (the host-side staging of
// each GPU is independent; no thread is created per call), returning the first non-zero status.
int for_each_gpu(CopyPool* workers, int G, const std::function<int(int)>& fn);

// The scratch of a measure pass (the clip stage's norm pass, the Krum and Bulyan stages' distance pass, the geomed
// stage's fused pass) on one GPU, grown on use (ensure_measure_scratch): `dev` holds room for `outs` fp64 results
// (a pass's sums or matrices, piece after piece) followed by `parts` per-workgroup partials, `host` is the pinned
// array the results are read back into.  One instance serves every stage and every part of a context, because
// every user waits on the host for the stream it enqueued on before it returns, the error returns included
// (measure_pass, measure_device): between two calls nothing on the device reads or writes it.
struct MeasureScratch {
    double* dev = nullptr;
    double* host = nullptr;
    size_t outs = 0, parts = 0;
};

struct GpuRes {
    int dev = 0;
    hipStream_t compute = nullptr, copy = nullptr, comm = nullptr;
    char* stage[2] = {nullptr, nullptr};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    int stage_i = 0;
    hipEvent_t copy_ev = nullptr;  // orders a reduction after the H2D copies queued on `copy`
    uint64_t copy_gen = 0;         // H2D batches queued on `copy` so far (a submit adds one)
    uint64_t copy_ev_gen = 0;      // the batch copy_ev was last recorded after
    std::map<hipStream_t, uint64_t> waited;  // per stream: the copy batch it last waited for
    hipEvent_t step_ev = nullptr;  // orders the rs exchange of a piece after its reduction
    void* scratch = nullptr;       // fp32 chain accumulator for a 16-bit output, D > kMaxClients
    MeasureScratch measure;        // the stages' measure passes (clip, Krum, geomed, Bulyan)
    // fa_output_crc32: the piece table (pinned staging + device copy) and the per-piece results, grown on use
    char* crc_host = nullptr;
    char* crc_dev = nullptr;
    size_t crc_bytes = 0;
    size_t scratch_bytes = 0;
    // Device segment tables of batched launches (fa_reduce_parts beyond the kernel-argument table): a ring,
    // so a changed table is uploaded into a slot whose last launch is long done; each slot remembers the
    // stream and event of its last launch, which orders a reuse or an overwrite after it (allocated on
    // first use).
    struct SegTable {
        fa::SegDesc* host = nullptr;  // pinned staging of the upload
        fa::SegDesc* dev = nullptr;
        hipEvent_t ev = nullptr;      // recorded after the slot's last launch (its upload precedes it)
        hipStream_t stream = nullptr; // the stream of that launch
        size_t bytes = 0;             // bytes of the table the slot holds
    };
    SegTable seg[kSegRing];
    int seg_last = -1;                // the slot of the last batched launch
    std::unique_ptr<CopyPool> pool;
    ncclComm_t nccl = nullptr;
};

// One copy-out run: elements [src, src + cnt) of a GPU's output buffer are bucket elements [dst, dst + cnt).
struct Run {
    size_t src, dst, cnt;
};

// One device allocation per GPU of the context (empty: none); both calls take each GPU's DeviceGuard.
struct DevArrays {
    std::vector<char*> p;
    explicit operator bool() const { return !p.empty(); }
    template <class T = char>
    T* at(size_t g) const { return reinterpret_cast<T*>(p[g]); }
    // hipMalloc of bytes(g) on every GPU.  -1, or the GPU it failed on after freeing what it made: the caller
    // reports FA_ERR_NOMEM in its own words.
    template <class Bytes>
    int alloc(const std::vector<GpuRes>& gpus, Bytes bytes) {
        p.assign(gpus.size(), nullptr);
        for (size_t g = 0; g < p.size(); ++g) {
            DeviceGuard dg(gpus[g].dev);
            if (hipMalloc((void**)&p[g], bytes(g)) == hipSuccess) continue;
            (void)hipGetLastError();
            p[g] = nullptr;
            free(gpus);
            return (int)g;
        }
        return -1;
    }
    void free(const std::vector<GpuRes>& gpus) {  // hipFree waits for the device's pending work
        for (size_t g = 0; g < p.size(); ++g) {
            DeviceGuard dg(gpus[g].dev);
            if (p[g]) (void)hipFree(p[g]);
        }
        p.clear();
    }
};

// ------------------------------------------------------------------ the stages (fa_stages.hip)
//
// A stage is its parameters (a Cfg with on(); the context holds one of each as the default of parts defined later,
// StageCfgs) and, in a part, that Cfg with its device arrays, its state across rounds and its last round's report.
// kRules (fa_stages.hip) holds its row of the admission rule.  What setting a stage does to a round under way:
//
//   stage            first set on a part                  set again          removed
//   opt clip noise   restart_round_plain                  the round stays    the round stays
//   krum geomed      restart_round_plain                  the round stays    the round stays (`ready` too)
//   bulyan           ready = false                        ready = false      ready = false, if it was on
//   mx8 reply        host_flush, restart_round_plain      nothing            the round stays
enum StageId { kOpt, kClip, kKrum, kGeomed, kBulyan, kNoise, kMx8, kReply, kStages };

struct OptCfg : fa_server_opt {  // fa.h "Server optimizer"
    OptCfg(const fa_server_opt& o = fa_server_opt{FA_OPT_NONE, 0.0f, 0.0f, 0.0f, 0.0f}) : fa_server_opt(o) {}
    bool on() const { return rule != FA_OPT_NONE; }
};
struct ClipCfg {  // fa.h "Clip stage"
    float max_norm = 0.0f;
    bool on() const { return max_norm > 0.0f; }
};
struct KrumCfg {  // fa.h "Krum stage"; m: as given in a default (-1: D - f), resolved in a part
    int f = 0, m = 0;
    bool on() const { return m != 0; }
};
struct GeomedCfg {  // fa.h "Geomed stage": T and nu
    int iters = 0;
    float nu = 0.0f;
    bool on() const { return iters != 0; }
};
struct BulyanCfg {  // fa.h "Bulyan stage"
    int f = -1;
    bool on() const { return f >= 0; }
};
struct NoiseCfg {  // fa.h "Noise stage"
    float stddev = 0.0f;
    uint64_t seed = 0;
    bool on() const { return stddev > 0.0f; }
};
struct FlagCfg {  // fa.h "MX8 receipts", "MX8 replies"
    bool flag = false;
    bool on() const { return flag; }
};
struct StageCfgs {
    OptCfg opt;
    ClipCfg clip;
    KrumCfg krum;
    GeomedCfg geomed;
    BulyanCfg bulyan;
    NoiseCfg noise;
    FlagCfg mx8, reply;
};

// Per GPU the fp32 state over its cnt elements (v only for the adaptive rules).
struct OptStage {
    OptCfg cfg;
    DevArrays x, m, v;
    bool master = false;  // x holds a model (set, or bootstrapped): the next reduction is a step
    uint64_t steps = 0;
    bool on() const { return cfg.on(); }
};
// Per GPU the fp32 reference over its cnt elements and, for a 16-bit input, the fp32 buffer the chain's first term
// fmaf(c0, g, +0) is written into.  The report: Q_k, the scales, who entered, how many were clipped.
struct ClipStage {
    ClipCfg cfg;
    DevArrays ref, init;
    bool has_ref = false;   // g holds a model (set, or left by a round): the next reduction clips
    bool reported = false;  // a reducing call ran with the stage: the arrays below describe it
    std::vector<double> q;
    std::vector<float> s;
    std::vector<int> in;
    int n = 0;
    bool on() const { return cfg.on(); }
};
// Host state only.  The report: the D x D matrix, the scores, the selection flags and their count.
struct KrumStage {
    KrumCfg cfg;
    bool reported = false;
    std::vector<double> q, s;
    std::vector<int> sel;
    int n = 0;
    bool on() const { return cfg.on(); }
};
// Host state only.  The trace: the valid passes, Q^t and alpha^t row by row, the objective per pass, the final flags.
struct GeomedStage {
    GeomedCfg cfg;
    bool reported = false;
    int passes = 0;
    std::vector<double> q, obj;
    std::vector<float> w;
    std::vector<int> in;
    bool on() const { return cfg.on(); }
};
// Host state only.  The report: the D x D matrix, the picks in pick order with their scores, the flags.
struct BulyanStage {
    BulyanCfg cfg;
    bool reported = false;
    std::vector<double> q, s;
    std::vector<int> order, sel;
    int n = 0;
    bool on() const { return cfg.on(); }
};
struct NoiseStage {
    NoiseCfg cfg;
    uint64_t round = 0;  // the round the next reducing call uses (2^32: that call is refused)
    bool on() const { return cfg.on(); }
};
// ref: the device output holds a reference -- a reducing call left it there while the stage was on, or
// fa_mx8_set_reference wrote it.  buf: per GPU the compressed shadows of its held slots, stride[g] bytes apart (q: cnt
// bytes, then from eoff[g] on the scale bytes of the blocks its range touches), allocated at the first fa_submit_mx8.
struct Mx8Stage {
    FlagCfg cfg;
    bool ref = false;
    DevArrays buf;
    std::vector<size_t> stride, eoff;
    bool on() const { return cfg.on(); }
};
// sent: per GPU the model the owners last received, cnt elements of the out dtype (has_sent: it holds one).  codes: per
// GPU the codes of the last reducing call, q (cnt bytes) and from eoff[g] on the scale bytes of the blocks its range
// touches (has_codes: that call was no bootstrap).  Allocated at the first reducing call with the stage on.
struct ReplyStage {
    FlagCfg cfg;
    bool has_sent = false, has_codes = false;
    DevArrays sent, codes;
    std::vector<size_t> eoff;
    bool counted = true;  // nan describes the codes above
    uint64_t nan = 0;
    bool on() const { return cfg.on(); }
};
// The stages that are on in a StageCfgs or a Part, one bit per StageId.
template <class S>
inline unsigned stages_on(const S& s) {
    return s.opt.on() << kOpt | s.clip.on() << kClip | s.krum.on() << kKrum | s.geomed.on() << kGeomed |
           s.bulyan.on() << kBulyan | s.noise.on() << kNoise | s.mx8.on() << kMx8 | s.reply.on() << kReply;
}

struct Part {
    int id = 0;  // its part_id (the noise stage's stream)
    size_t n = 0;
    fa_dtype in = FA_F32, out = FA_F32;
    int D = 0;
    fa_mode mode = FA_FEDAVG;
    float divisor = FA_DEFAULT_DIVISOR;
    int trim = FA_TRIM_MEDIAN;     // FA_TRIMMED: as given to fa_set_trim (resolved against D at each reduction)
    bool rs = false;               // FA_SHARD_CLIENT_RS layout
    size_t npad = 0;               // rs: slot length (n padded to a multiple of G * 64)
    std::vector<size_t> off, cnt;  // per GPU: bucket elements held by its slots (range: its shard; rs: [0, n))
    std::vector<int> c0, c1;       // per GPU: the client slots it holds, [c0, c1)
    std::vector<char*> pool;       // per GPU: its client slots + the output (+ rs partial, eager acc)
    std::vector<size_t> stride;    // per GPU: bytes between consecutive slots of one piece
    // Pieces (range layout): a GPU whose slots would span more than 48 GiB (piece_len_for) holds its range as
    // npiece[g] pieces of piece_len[g] elements (the last one shorter): piece j of every slot lies in the
    // j-th region of the pool (slots of one piece stride[g] apart), so one launch reads clients that lie
    // close together (the address span).  One piece = the plain layout.
    std::vector<int> npiece;
    std::vector<size_t> piece_len;
    std::vector<void*> dout;       // per GPU: the output (range: cnt elements of `out`; rs: its fp32 shard)
    std::vector<void*> dout16;     // rs with a 16-bit output: per GPU, its shard rounded to it (the copy-out's source)
    std::vector<float*> partial;   // rs: per GPU, fp32 partial over its clients, npad elements
    std::vector<float*> acc;       // FA_ACCUMULATE_ON_ARRIVAL: per GPU, fp32 chain of the reduced prefix
    std::vector<hipEvent_t> done;  // per GPU: orders the copy-out after the reduction (see mark_done)
    std::vector<hipStream_t> done_stream;  // per GPU: the stream the last reduction ran on
    std::vector<float> w;
    std::vector<char> submitted;
    int n_submitted = 0;
    int last_slot = -1;
    int reduced = 0;    // accumulate on arrival: slots [0, reduced) are chained into acc (or dout)
    bool ready = false; // this round's output is reduced already (eager prefix reached D, fa_reduce_parts)
    std::vector<std::vector<Run>> runs;  // per GPU: where its output goes (set by the last reduction)
    std::vector<void*> run_src;          // per GPU: the buffer the runs read
    // Small receipts kept where they arrived (host_keep): per slot the receipt's pinned segments -- the host
    // address (for a later DMA, host_flush) and the address a kernel reads it at -- empty = in the slot.
    struct HostSeg {
        const char* host;
        const char* dev;
        size_t bytes;
    };
    std::vector<std::vector<HostSeg>> host_src;
    int n_host = 0;  // slots whose receipt is kept host-side this round
    // The stages (above), and for a 16-bit output the fp32 buffer the round's aggregate is reduced into, per GPU:
    // there while the part has a server-optimizer or a noise stage (ensure_oavg, drop_oavg_if_unused).
    OptStage opt;
    ClipStage clip;
    KrumStage krum;
    GeomedStage geomed;
    BulyanStage bulyan;
    NoiseStage noise;
    Mx8Stage mx8;
    ReplyStage reply;
    DevArrays oavg;
};

// A part whose reducing calls are rounds of their own (any stage but MX8 receipts): never batched, eager or
// host-read, every client submitted before each.
inline bool staged(const Part& p) { return (stages_on(p) & ~(1u << kMx8)) != 0; }
// A part that gets its first stage: what this round chained or kept host-side so far goes back to the plain path.
inline void restart_round_plain(Part& p) {
    p.reduced = 0;
    p.ready = false;
}

}  // namespace fah

struct fa_ctx {
    int G = 1;
    int flags = 0;
    float divisor = FA_DEFAULT_DIVISOR;
    int trim = FA_TRIM_MEDIAN;  // default of FA_TRIMMED parts defined later
    fah::StageCfgs defaults;    // default stages of the parts defined later that take them (taken_defaults)
    fah::CtxTuning tuning;
    std::vector<fah::GpuRes> gpu;
    std::map<int, fah::Part> parts;
    std::unique_ptr<fah::CopyPool> workers;  // G > 1: one persistent host thread per GPU (for_each_gpu)
    unsigned long long host_reads = 0;       // reductions that read their receipts in place (fa_diag_host_reads)
};

namespace fah {

// What a fa_*_device entry runs on (gpu checked against ctx->G before): the ctx's GPU `gpu`, hip_stream or that
// GPU's compute stream, the ctx's tuning; without a ctx HIP device `gpu`, the defaults, g = 0.  No device call.
struct DeviceCall {
    int dev, g;
    hipStream_t s;
    fa::Tuning tu;
};
DeviceCall device_call(fa_ctx* ctx, int gpu, void* hip_stream);

// FA_TRIMMED: the trim a reduction over D clients uses (FA_TRIM_MEDIAN -> (D-1)/2); a mode's kernel argument.
inline int resolved_trim(int trim, int D) { return trim == FA_TRIM_MEDIAN ? (D - 1) / 2 : trim; }
inline float mode_arg(fa_mode mode, float divisor, int trim, int D) {
    return mode == FA_TRIMMED ? (float)resolved_trim(trim, D) : divisor;
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }
// A client pointer array (`what`: "client", "client slot"): there, every entry non-null and aligned to its element.
int check_clients(const void* const* ptrs, int D, size_t elem, const char* what);
// Clients [k0, k0 + nc) of ptrs with their weights (w null: 0.0f, for the launches that read none).
fa::ClientTable client_table(const void* const* ptrs, const float* w, int k0, int nc);
// The device reduction for one GPU, shared by every entry: D clients (any D >= 1; more than kMaxClients
// continue the chain from an fp32 accumulator in further passes) -> dst.  `divisor` is the mode's parameter:
// FA_LITERAL's divisor, or FA_TRIMMED's resolved trim (mode_arg: a small integer, exact as a float).
int reduce_on(fa_ctx* ctx, int g, const fa::Tuning& tu, const void* const* clients, const float* w, int D, size_t n,
              fa_dtype in, void* dst, fa_dtype out, fa_mode mode, float divisor, const float* init, hipStream_t s);

inline bool holds(const Part& p, int g, int k) { return k >= p.c0[(size_t)g] && k < p.c1[(size_t)g]; }
// Piece j of GPU g: GPU-local elements [piece_lo, piece_lo + piece_cnt), the slot of client k at piece_ptr.
inline size_t piece_lo(const Part& p, int g, int j) { return (size_t)j * p.piece_len[(size_t)g]; }
inline size_t piece_cnt(const Part& p, int g, int j) {
    const size_t lo = piece_lo(p, g, j), n = p.cnt[(size_t)g];
    return lo >= n ? 0 : std::min(p.piece_len[(size_t)g], n - lo);
}
inline char* piece_ptr(const Part& p, int g, int k, int j) {
    const size_t held = (size_t)(p.c1[(size_t)g] - p.c0[(size_t)g]);
    return p.pool[(size_t)g] + ((size_t)j * held + (size_t)(k - p.c0[(size_t)g])) * p.stride[(size_t)g];
}
inline char* slot_ptr(const Part& p, int g, int k) { return piece_ptr(p, g, k, 0); }  // one-piece parts
// The pointer list of piece j of GPU g over clients [k0, k1), in a vector the caller keeps across pieces.
template <typename P>
P* const* piece_ptrs(const Part& p, int g, int j, int k0, int k1, std::vector<P*>& out) {
    out.resize((size_t)(k1 - k0));
    for (int k = k0; k < k1; ++k) out[(size_t)(k - k0)] = piece_ptr(p, g, k, j);
    return out.data();
}

// fa_api.hip, for the stages (each is described where it is defined)
int check_part(fa_ctx* ctx, int part_id, Part** out);
int wait_copies(fa_ctx* ctx, int g, hipStream_t s);
void set_range_runs(Part& p, int G);
int host_flush(fa_ctx* ctx, Part& p);
int mark_submitted(fa_ctx* ctx, Part& p, int slot, float weight);
int reduce_part(fa_ctx* ctx, Part& p, const float* w, hipStream_t s);
void reset_round(Part& p);

// fa_stages.hip, for the rest of the library.  The defaults a new part of `mode` with D clients takes, as bits per
// StageId, after the D-dependent checks of those it takes (*c: the defaults, Krum's m resolved); one of them, or a
// setter's request, applied to a part; everything the stages hold in a part, freed.
int taken_defaults(const fa_ctx* ctx, fa_mode mode, int D, StageCfgs* c, unsigned* taken);
int set_part_stage(fa_ctx* ctx, Part& p, StageId id, const StageCfgs& c);
void free_stages(fa_ctx* ctx, Part& p);
void free_measure_scratch(MeasureScratch& m);

// What a measure-then-select stage makes of a round (fa.h "Clip stage", rules 1-3; "Krum stage", rules 1-4): the
// clients that enter the chain in ascending order, their weights w'_k, and the weight c0 of the clip reference
// as the chain's first term (0: none, as always for Krum).
struct SubsetPlan {
    std::vector<int> inc;
    std::vector<float> w;
    float c0 = 0.0f;
};
// One reducing call of a range part as its stages see it (reduce_part keeps the loops over GPUs and pieces).  Begin:
// the noise stage's round budget, the clip report reset, the plan of the family stage or of Bulyan with its measure
// passes and host waits.  One piece, on the current device: the aggregate (the plain chain, the plan's chain or
// Bulyan's centred mean), then noise, then the optimizer's step or bootstrap, then the clip reference unless a reply
// stage follows.  The end of a GPU: the reply stage, then the clip references from g'.  The end: the state across rounds.
struct StageRound {
    SubsetPlan plan;
    bool subset = false;  // the aggregate is the plan's chain: a clip stage with a reference, Krum, geomed
};
int stage_round_begin(fa_ctx* ctx, Part& p, const float* w, hipStream_t s, StageRound* rd);
int stage_piece(fa_ctx* ctx, Part& p, int g, int j, const float* w, const StageRound& rd, std::vector<const void*>& ptrs,
                hipStream_t st);
int stage_gpu_end(fa_ctx* ctx, Part& p, int g, hipStream_t st);
void stage_round_end(Part& p);

}  // namespace fah
