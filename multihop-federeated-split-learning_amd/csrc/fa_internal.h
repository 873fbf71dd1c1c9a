// fa_internal.h -- shared declarations between the kernel TU and the C-ABI TU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_split.h"
#include "fedavg/fa.h"

namespace fa {

// The (input, output) dtype pairs the library reduces: a bucket keeps its dtype, widens to fp32 or is rounded
// from fp32.  The two 16-bit formats never convert into each other (bf16 <-> fp16 is refused, FA_ERR_ARG).
inline bool dtype_pair_ok(fa_dtype in, fa_dtype out) { return in == out || in == FA_F32 || out == FA_F32; }
inline const char* dtype_name(fa_dtype t) { return t == FA_F32 ? "f32" : t == FA_BF16 ? "bf16" : "f16"; }

// Clients per launch.  Pointers + weights travel in the kernel-argument segment
// (1.5 KiB of the 4 KiB kernarg segment), read with scalar loads; more clients continue the chain in
// another pass.  128 covers C5 (D = 128) in one pass.
constexpr int kMaxClients = 128;

struct ClientTable {
    const void* src[kMaxClients];
    float w[kMaxClients];
};

// One bucket of a batched launch (fedavg_segments_kernel): workgroups [blk0, blk0 + nblk) of the grid
// reduce its nvec 16-byte vectors, the last of them also the scalar tail [nvec * V, n).  Device memory.
struct SegDesc {
    int64_t blk0, nblk, nvec, n;
    void* out;
    int nc, pad;
    const void* src[kMaxClients];
    float w[kMaxClients];
};

// A small batch in the kernel arguments: segment s = workgroups [blk0[s], blk0[s+1]), its clients are
// src/w[src0[s], src0[s] + nc[s]).
constexpr int kSegArgMax = 8, kSegArgClients = 192;
struct SegArgs {
    int nseg;
    int nc[kSegArgMax], src0[kSegArgMax];
    int64_t blk0[kSegArgMax + 1], nvec[kSegArgMax], n[kSegArgMax];
    void* out[kSegArgMax];
    const void* src[kSegArgClients];
    float w[kSegArgClients];
};

struct Tuning {
    int block;       // threads per workgroup: 64, 128 or 256
    int max_blocks;  // grid cap (grid-stride beyond it), <= 0: uncapped
    int unroll;      // clients per load group: 4, 8, 16
    int load_nt;      // non-temporal client loads
    int store_policy; // 0 plain, 1 nt, 2 sc1 (write-through), 3 sc0 sc1
    int walk;         // FedAvg grid walk: 0 linear, 1 XCD eighths, 2 XCD eighths, odd ones reversed,
                      // 3 phased (persistent grid, reads and writes separated in time; XCD eighths
                      // for buckets smaller than one phase), 4 phased with the larger register stage
};

// CRC-32 of byte ranges of device memory (the reply's zip records): piece i = [base + off[i], + len[i]),
// chunk0 the prefix count of its 256-byte chunks (np + 1 entries, chunks = chunk0[np]); out[i] (zeroed by the
// caller) gets R(piece i, 0), the CRC register over the piece from 0, without the inversions.  Device arrays.
hipError_t launch_crc32_pieces(const void* base, const uint64_t* d_off, const uint64_t* d_len, const uint64_t* d_chunk0,
                               int np, uint64_t chunks, uint32_t* d_out, hipStream_t s);
constexpr uint64_t kCrcChunkBytes = 256;
// Host side of the same algebra: a * b mod P (reflected) and x^(8 n) mod P.
uint32_t crc32_mulmod(uint32_t a, uint32_t b);
uint32_t crc32_x8n(uint64_t n);

hipError_t launch_chain(const ClientTable& t, int nc, fa_dtype in, fa_dtype out, const float* init, void* dst,
                        const Split& sp, const Tuning& tu, hipStream_t s);
// Meetings of the phased kernel on device `dev` that gave up waiting (the grid was not co-resident).
hipError_t phased_timeouts(int dev, uint64_t* count);
// FA_TIMELINE=1 diagnostic: copies the last phased launch's per-workgroup timeline (8 words each) on device
// dev into out; returns the words copied (0: no timeline, -1: HIP error).
int phased_timeline(int dev, unsigned long long* out, int cap);
// The phased kernel's counter slot of stream s on device dev (assigned on first use, as a launch would;
// *own: the slot is the stream's alone), and the release of a stream's owned slot (fa_destroy).
int phased_slot(int dev, hipStream_t s, bool* own);
void phased_release_stream(int dev, hipStream_t s);
int phased_owned_slots(int dev);  // owned slots currently taken on dev
// What one FedAvg chain launch runs (plan_chain, host-only): the one-shot vector grid, the one-element-per-
// lane kernel (mixed 16-byte phases), or the phased persistent grid (`threads` per workgroup, `regs` bytes of
// register stage per lane, `phases` phases; phases > 1 means chip-wide meetings).
enum { kPlanOneShot = 0, kPlanScalar = 1, kPlanPhased = 2 };
struct ChainPlan {
    int kind, regs, threads;
    int64_t phases;
};
// cus: the device's CU count (0 = no phased kernel).
ChainPlan plan_chain(fa_dtype in, fa_dtype out, int64_t nvec, int nc, bool vector_ok, const Tuning& tu, int cus);
hipError_t launch_literal(const void* x, fa_dtype in, void* dst, fa_dtype out, float divisor,
                          const Split& sp, const Tuning& tu, hipStream_t s);
// Coordinate-wise trimmed mean over t.src[0..nc), 1 <= nc <= FA_TRIMMED_MAX_CLIENTS, 0 <= 2 trim < nc (fa.h "FA_TRIMMED"):
// sorted positions [trim, nc - trim) of every element, added ascending from +0, divided by nc - 2 trim.
// Weights are not read.  fa_trimmed.hip.
hipError_t launch_trimmed(const ClientTable& t, int nc, fa_dtype in, fa_dtype out, int trim, void* dst,
                          const Split& sp, const Tuning& tu, hipStream_t s);
// The Bulyan stage's centred mean (fa.h "Bulyan stage", rule 4), fa_centered.hip: per element the mean of the
// `keep` values (1 <= keep <= nc) closest to the median of the nc clients' values, nc <= FA_TRIMMED_MAX_CLIENTS.
// Arguments, dtype pairs, forms and stores as launch_trimmed.
hipError_t launch_centered(const ClientTable& t, int nc, fa_dtype in, fa_dtype out, int keep, void* dst,
                           const Split& sp, const Tuning& tu, hipStream_t s);
// The server-optimizer stage (fa.h "Server optimizer"), fa_server_opt.hip.  One step of `rule` (an fa_opt_rule
// other than FA_OPT_NONE, or kOptBoot: x' = avg, m' = v' = +0, v nullable) over n elements: reads avg and the
// fp32 state x, m, v (v null and untouched for FA_OPT_MOMENTUM), writes the state and, unless out is null, x'
// in dtype `odt`.  out may be avg itself for FA_F32.  sp: the Split (fa_split.h) led by avg, 4 elements per
// vector.
constexpr int kOptBoot = 0;
struct OptHyper {
    float lr, beta1, beta2, tau;
    float c1, c2;  // fl(1 - beta1), fl(1 - beta2), computed on the host
};
hipError_t launch_server_opt(int rule, const OptHyper& h, const float* avg, float* x, float* m, float* v, void* out,
                             fa_dtype odt, const Split& sp, const Tuning& tu, hipStream_t s);
// The clip stage's norm pass (fa.h "Clip stage"), fa_clip.hip.  sums[k] = sum_i ((double)fl32(x_{k,i} - ref_i))^2
// over the n elements of clients t.src[0..nc), 1 <= nc <= kMaxClients (weights not read): one launch over all
// clients writes one fp64 partial per (client, workgroup) into `partials` (room for nc * kClipMaxPartials
// doubles; a client's are the np of measure_grid, fa_split.h, stored np apart), a second one adds each client's
// partials in a fixed order.  No atomics.  sp: the Split (fa_split.h) led by the first client, ref required as
// well.  The caller's scratch holds results and partials of either pass (MeasureScratch, fa_host.h).
constexpr int64_t kClipMaxBlocks = 2048;  // 8 workgroups per CU on 256 CUs; tiles beyond it are strided
constexpr int64_t kClipMaxPartials = kClipMaxBlocks + 1;  // per client: the grid's, plus one for head and tail
hipError_t launch_clip_sumsq(const ClientTable& t, int nc, fa_dtype in, const float* ref, const Split& sp,
                             double* partials, double* sums, const Tuning& tu, hipStream_t s);
// The second launch of a measure pass (fa_clip.hip; shared with fa_geomed.hip): sums[r] = the np partials of row r <
// rows, stored np apart, one wave per row, lane l adding partials l, l + 64, ... in ascending order.
hipError_t launch_measure_finish(const double* partials, int64_t np, int rows, double* sums, hipStream_t s);
// The geomed stage's fused Weiszfeld pass (fa.h "Geomed stage", rule 1), fa_geomed.hip.  Per element v_i = the
// FA_FEDAVG chain over clients t.src[0..nc) with weights t.w, 1 <= nc <= kMaxClients, held in registers; sums[k] =
// Q_k = sum_i ((double)fl32(x_{k,i} - v_i))^2 and sums[nc + k] = B_k = the count of elements of client k that are
// NaN or +-inf, over the n elements.  The buckets are read once; v is stored only if v_out (fp32, n elements) is
// given.  One launch writes one fp64 partial per (row, workgroup) into `partials` (room for 2 nc *
// kClipMaxPartials doubles, laid out as the clip pass's), launch_measure_finish adds them.  No atomics.  sp: the
// Split (fa_split.h) led by the first client, v_out required as well if given.
hipError_t launch_geomed_pass(const ClientTable& t, int nc, fa_dtype in, float* v_out, const Split& sp, double* partials,
                              double* sums, const Tuning& tu, hipStream_t s);
// dst[i] = src[i] widened to fp32 exactly (the part's output into its reference; signed zeros kept).
hipError_t launch_clip_widen(const void* src, fa_dtype dt, float* dst, int64_t n, hipStream_t s);
// The Krum stage's distance pass (fa.h "Krum stage", rule 1), fa_krum.hip.  dist (device, D * D doubles, row-major)
// := Q_ab = sum_i ((double)fl32(x_{a,i} - x_{b,i}))^2 over the n elements of clients t.src[0..D), 1 <= D <=
// kMaxClients (weights not read), each pair computed once and mirrored, the diagonal +0: one launch over all
// clients writes one fp64 partial per (pair, workgroup) into `partials` (room for krum_pairs(D) *
// kKrumMaxPartials doubles, laid out as the clip pass's; not read for D == 1), a second one adds each pair's
// partials in a fixed order.  No atomics.  sp: the Split (fa_split.h) led by the first client.
constexpr int64_t kKrumMaxBlocks = 1024;  // 4 workgroups of 34 KiB LDS per CU on 256 CUs; tiles beyond it are strided
constexpr int64_t kKrumMaxPartials = kKrumMaxBlocks + 1;  // per pair: the grid's, plus one for head and tail
inline int64_t krum_pairs(int D) { return (int64_t)D * (D - 1) / 2; }
hipError_t launch_pairdist(const ClientTable& t, int D, fa_dtype in, const Split& sp, double* partials, double* dist,
                           const Tuning& tu, hipStream_t s);
// The noise stage (fa.h "Noise stage"), fa_noise.hip.  out[i] (dtype odt, one rounding) := fl(avg[i] + fl(stddev z_i))
// over n elements, z_i the unit normal of bucket element idx0 + i under (seed, stream, round): the result does not
// depend on how a bucket is cut into launches.  out may be avg itself for FA_F32.  sp: the Split (fa_split.h) led by
// avg, 4 elements per vector, out required as well.
hipError_t launch_noise(const float* avg, void* out, fa_dtype odt, float stddev, uint64_t seed, uint32_t stream,
                        uint32_t round, uint64_t idx0, const Split& sp, const Tuning& tu, hipStream_t s);
// The same normals on the host (fa_noise_host): z[0, n) := z_{idx0} .. z_{idx0 + n - 1}.  The kernel's own source.
void noise_host(uint64_t seed, uint32_t stream, uint32_t round, uint64_t idx0, size_t n, float* z);
// MX8 receipts (fa.h "MX8 receipts"), fa_mx8.hip.  dst[i] (dtype ddt, one rounding) := fl(widen(ref[i]) + d_i), or d_i
// without a reference (ref null), over n elements, d_i = fl((float)q[i] * 2^(E - 133)) with E = e[((idx0 + i) >> 5) -
// (idx0 >> 5)]: e[0] is the scale of the block that bucket element idx0 lies in.  (ddt, rdt) as dtype_pair_ok(in, out).
// Any pointers of element alignment: mx8_split (host-only) says which form a launch takes.
Split mx8_split(const void* q, size_t n, const void* ref, fa_dtype rdt, const void* dst, fa_dtype ddt);
hipError_t launch_mx8_expand(const int8_t* q, const uint8_t* e, uint64_t idx0, int64_t n, const void* ref, fa_dtype rdt,
                             void* dst, fa_dtype ddt, hipStream_t s);
// The codec on the host (fa_mx8_decode: the kernel's own multiply and scale; fa_mx8_encode: the owner's side).
void mx8_decode_host(const int8_t* q, const uint8_t* e, size_t n, uint64_t idx0, float* d);
void mx8_encode_host(const float* delta, size_t n, int8_t* q, uint8_t* e);
// MX8 replies (fa.h "MX8 replies"), fa_mx8_enc.hip.  Over n elements of dtype dt: delta_i = fl(widen(y[i]) -
// widen(sent[i])); mode 0 (fused): e := the scales of the blocks of bucket elements [idx0, idx0 + n) from the deltas
// of this launch (e[0]: block idx0 >> 5), q := their codes, and out, out2 (each nullable) := g' = fl(widen(sent[i]) +
// d_i), rounded once to dt; mode 1 (scales only): e alone is written; mode 2 (scales given): e is read, the rest as
// mode 0.  out and out2 may each be y or sent exactly (a lane reads its elements before it writes any); q and e
// overlap nothing.  Any pointers of element alignment: mx8_enc_split (host-only) says which form a fused launch takes.
enum { kMx8EncFused = 0, kMx8EncScalesOnly = 1, kMx8EncScalesGiven = 2 };
Split mx8_enc_split(const void* y, const void* sent, fa_dtype dt, uint64_t idx0, size_t n, const void* q,
                    const void* out, const void* out2);
hipError_t launch_mx8_encode(const void* y, const void* sent, fa_dtype dt, uint64_t idx0, int64_t n, int8_t* q,
                             uint8_t* e, void* out, void* out2, int mode, hipStream_t s);
// In-place state sync: every slot t.src[0..nc) := the chain over them (continuing `init` if given).
hipError_t launch_sync(const ClientTable& t, int nc, fa_dtype dt, const float* init, const Split& sp,
                       const Tuning& tu, hipStream_t s);
// slots t.src[0..nc) := acc (rounded to dt).
hipError_t launch_broadcast(const ClientTable& t, int nc, fa_dtype dt, const float* acc, int64_t n,
                            const Tuning& tu, hipStream_t s);
// One launch over nseg buckets (FedAvg, no init, every pointer 16-byte aligned); blocks = sum of nblk.
hipError_t launch_segments(const SegDesc* d_segs, int nseg, int64_t blocks, fa_dtype in, fa_dtype out, int max_nc,
                           const Tuning& tu, hipStream_t s);
// The same with the table in the kernel arguments (a.nseg <= kSegArgMax, sum of nc <= kSegArgClients).
hipError_t launch_segargs(const SegArgs& a, fa_dtype in, fa_dtype out, int max_nc, const Tuning& tu, hipStream_t s);
// Whether launch_chain takes the phased kernel for a bucket of nvec vectors and nc clients.
bool phased_takes(fa_dtype in, fa_dtype out, int64_t nvec, int nc, const Tuning& tu);
hipError_t launch_fill(void* dst, int64_t n, fa_dtype dt, uint64_t seed, uint32_t client, uint64_t idx0,
                       hipStream_t s);
// Read-stream probe over nc f32 buffers of nvec 16-byte vectors (16-byte aligned); nothing is written.
hipError_t launch_read_probe(const ClientTable& t, int nc, int64_t nvec, float* sink, hipStream_t s);
hipError_t launch_read_plain(const ClientTable& t, int nc, int64_t nvec, int grid, int unroll, float* sink,
                             hipStream_t s);
hipError_t launch_rw_plain(const ClientTable& t, int nc, int64_t nvec, int grid, int unroll, bool nt, hipStream_t s);

}  // namespace fa
