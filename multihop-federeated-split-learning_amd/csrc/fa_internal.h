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
// The Gram pass (fa.h "Gram pass"), fa_gram.hip.  gram (device, D * D doubles, row-major) := G_ab = sum_i (double)y_a,i
// (double)y_b,i over the n elements of clients t.src[0..D), 1 <= D <= kMaxClients (weights not read), y the widened
// input or, with ref (n fp32, nullable), fl32(widen(x) - ref_i); each entry a <= b computed once on the fp64 MFMA and
// mirrored, the diagonal included.  One launch over tiles of gram_tile(ceil(D / 16)) elements of all clients writes one
// fp64 partial per (entry, workgroup) into `partials` (room for gram_entries(D) * kGramMaxPartials doubles, laid out
// as the clip pass's), a second one adds each entry's partials in a fixed order.  No atomics.  sp: the Split
// (fa_split.h) led by the first client, ref required as well if given.
constexpr int64_t kGramMaxBlocks = 768;  // 3 workgroups per CU on 256 CUs, resident at once in every form (at 97 .. 128
                                         // clients the vector form holds 3 waves per SIMD); tiles beyond it are strided
constexpr int64_t kGramMaxPartials = kGramMaxBlocks + 1;  // per entry: the grid's, plus one for head and tail
inline int64_t gram_entries(int D) { return (int64_t)D * (D + 1) / 2; }
constexpr int gram_tile(int B) { return B == 1 ? 256 : B == 2 ? 128 : B <= 4 ? 64 : 32; }  // elements per tile at B blocks
hipError_t launch_gram(const ClientTable& t, int D, fa_dtype in, const float* ref, const Split& sp, double* partials,
                       double* gram, const Tuning& tu, hipStream_t s);
// The noise stage (fa.h "Noise stage"), fa_noise.hip.  out[i] (dtype odt, one rounding) := fl(avg[i] + fl(stddev z_i))
// over n elements, z_i the unit normal of bucket element idx0 + i under (seed, stream, round): the result does not
// depend on how a bucket is cut into launches.  out may be avg itself for FA_F32.  sp: the Split (fa_split.h) led by
// avg, 4 elements per vector, out required as well.
hipError_t launch_noise(const float* avg, void* out, fa_dtype odt, float stddev, uint64_t seed, uint32_t stream,
                        uint32_t round, uint64_t idx0, const Split& sp, const Tuning& tu, hipStream_t s);
// The same normals on the host (fa_noise_host): z[0, n) := z_{idx0} .. z_{idx0 + n - 1}.  The kernel's own source.
void noise_host(uint64_t seed, uint32_t stream, uint32_t round, uint64_t idx0, size_t n, float* z);
// The secagg stage (fa.h "Secagg stage"), fa_secagg.hip.  out[i] := fl32((float)(int32_t)u_i * scale) rounded once to
// odt, u_i = init[i] + the nc buckets' words + the signed ChaCha20 words of the T terms at bucket element idx0 + i,
// modulo 2^32 (raw: out[i] := u_i as uint32, no terms, the sums a later pass continues; out may be init).  tab: the
// device copy of secagg_table's words, with npos and cnet as it gave them.  sp: secagg_split of the first bucket,
// every other bucket and out required as well.  form: kSecaggTile or kSecaggSplit, anything else = secagg_form(n, T).
enum { kSecaggTile = 0, kSecaggSplit = 1 };
int secagg_form(int64_t n, int T);  // host rule: which vector form a launch over n elements and T terms takes
// The split of a launch over bucket elements [idx0, idx0 + n) whose first bucket lies at `lead` (host-only): the head
// ends at a multiple of 16 of the bucket index, which brings `lead` to 16 bytes iff the two phases agree modulo 4;
// else the launch takes the element form throughout.
Split secagg_split(const void* lead, uint64_t idx0, size_t n);
// The term table (host-only): tab (secagg_table_words(T) words) := the uniform sums of the initial states, then the
// terms (key: 8 words each, nonce: 3) with the +1 terms first; *npos their count, *cnet = npos - (T - npos).
size_t secagg_table_words(int T);
void secagg_table(int T, const uint32_t* keys, const uint32_t* nonces, const int* signs, uint32_t* tab, int* npos,
                  uint32_t* cnet);
hipError_t launch_secagg(const ClientTable& t, int nc, const uint32_t* tab, int T, int npos, uint32_t cnet,
                         const uint32_t* init, void* out, fa_dtype odt, bool raw, float scale, uint64_t idx0,
                         const Split& sp, int form, const Tuning& tu, hipStream_t s);
// The mask words on the host (fa_secagg_mask_host): out[0, n) := the words of elements idx0 .. idx0 + n - 1.  The
// kernel's own rounds.
void secagg_mask_host(const uint32_t* key, const uint32_t* nonce, uint64_t idx0, size_t n, uint32_t* out);
// The sign-vote stage (fa.h "Sign-vote stage"), fa_sign.hip.  out[i] (dtype odt, one rounding) := fl32(widen(ref[i]) + t_i),
// or t_i with ref null, over n elements whose bits are bit i & 31 of word i >> 5 of bits[0..D) (each pointer at the word of
// the launch's first element, a multiple of 32 of the bucket index); neg, pos (both or neither, majority only): the vote
// planes, (n + 31) / 32 words each.  (rdt, odt) as dtype_pair_ok(in, out); out may be ref exactly (a lane reads its
// elements before it writes them).  sp: sign_split of the same operands (host-only): the words before the receipts' 16-byte
// boundary, the quads of 128 elements the vector form takes, and whether it may (one 16-byte phase of all receipts and of
// the planes; ref, out 16-byte aligned).
struct SignSplit {
    int64_t headw, nq, nwords;
    bool vec;
    int64_t tailw0() const { return headw + 4 * nq; }
    int64_t edge_words() const { return headw + (nwords - tailw0()); }  // words left to the element form
};
SignSplit sign_split(const uint32_t* const* bits, int D, size_t n, const void* ref, fa_dtype rdt, const void* out,
                     fa_dtype odt, const void* neg, const void* pos);
hipError_t launch_sign_vote(const uint32_t* const* bits, int D, int64_t n, float eta, int rule, int margin, const void* ref,
                            fa_dtype rdt, void* out, fa_dtype odt, uint32_t* neg, uint32_t* pos, const SignSplit& sp,
                            const Tuning& tu, hipStream_t s);
// The rule on the host (fa_sign_pack, fa_sign_vote_host): plain loops; bits[k] are whole receipts, element i is bucket
// element idx0 + i, ref / out / neg / pos are the range's own.
void sign_pack_host(const float* delta, size_t n, uint32_t* bits);
void sign_vote_host(const uint32_t* const* bits, int D, size_t n, uint64_t idx0, float eta, int rule, int margin,
                    const float* ref, float* out, uint32_t* neg, uint32_t* pos);
// The sparse-sum stage (fa.h "Sparse-sum stage"), fa_sparse.hip.  out[i] (dtype odt, one rounding) := fl32(widen(ref[i]) +
// acc_i), or acc_i with ref null, over n elements, bucket elements idx0 .., acc_i the fmaf chain over the entries (idx[c][j],
// val[c][j]), j < k[c] <= 2^32 - 1, of clients c = 0 .. D - 1 in that order under w[c].  (rdt, odt) as dtype_pair_ok(in,
// out); out may be ref exactly (a lane reads its elements before it writes them).  work: sparse_workspace(n, D) bytes,
// 4-byte aligned, not initialised.  form: kSparseSmall or kSparseBig, the tile a wave owns; anything else =
// sparse_tile_form(k, D, n), by density.  sparse_vec: whether the dense side may use 16-byte accesses (host-only).
enum { kSparseSmall = 0, kSparseBig = 1 };
constexpr int kSparseTileSmall = 2048, kSparseTileBig = 8192;
constexpr int kSparseGroup = 4;  // the clients whose first entries a wave keeps in flight
int sparse_tile_form(const uint64_t* k, int D, size_t n);
bool sparse_vec(size_t n, const void* ref, fa_dtype rdt, const void* out, fa_dtype odt);
size_t sparse_workspace(size_t n, int D);
hipError_t launch_sparse_sum(const uint32_t* const* idx, const float* const* val, const uint64_t* k, const float* w, int D,
                             uint64_t idx0, int64_t n, const void* ref, fa_dtype rdt, void* out, fa_dtype odt, void* work,
                             int form, const Tuning& tu, hipStream_t s);
// Rules 1-2 on the host (fa_sparse_sum_host): plain loops, client by client.
void sparse_sum_host(const uint32_t* const* idx, const float* const* val, const uint64_t* k, const float* w, int D, size_t n,
                     uint64_t idx0, const float* ref, float* out);
// MX8 receipts (fa.h "MX8 receipts"), fa_mx8.hip.  dst[i] (dtype ddt, one rounding) := fl(widen(ref[i]) + d_i), or d_i
// without a reference (ref null), over n elements, d_i = fl((float)q[i] * 2^(E - 133)) with E = e[((idx0 + i) >> 5) -
// (idx0 >> 5)]: e[0] is the scale of the block that bucket element idx0 lies in.  (ddt, rdt) as dtype_pair_ok(in, out).
// Any pointers of element alignment: mx8_split (host-only) says which form a launch takes.
Split mx8_split(const void* q, size_t n, const void* ref, fa_dtype rdt, const void* dst, fa_dtype ddt);
hipError_t launch_mx8_expand(const int8_t* q, const uint8_t* e, uint64_t idx0, int64_t n, const void* ref, fa_dtype rdt,
                             void* dst, fa_dtype ddt, hipStream_t s);
// The MX8-sum stage (fa.h "MX8-sum stage"), fa_mx8sum.hip.  out[i] (dtype odt, one rounding) := fl32(widen(ref[i]) + acc_i),
// or acc_i with ref null, over n elements, bucket elements idx0 .., acc_i the fmaf chain over d_c,i = fl((float)q[c][i] *
// 2^(E - 133)), E = e[c][((idx0 + i) >> 5) - (idx0 >> 5)], of clients c = 0 .. D - 1 in that order under w[c].  (rdt, odt) as
// dtype_pair_ok(in, out); out may be ref exactly (a lane reads its elements before it writes them).  Any pointers of
// element alignment: mx8sum_split (host-only) says which form a launch takes (vec: the vector form over [head, tail0)).
constexpr int kMx8SumTile = 4096;  // the elements of a workgroup's tile: 128 blocks
constexpr int kMx8SumGroup = 4;    // the clients whose q words a lane keeps in flight
Split mx8sum_split(size_t n, const int8_t* const* q, int D, uint64_t idx0, const void* ref, fa_dtype rdt, const void* out,
                   fa_dtype odt);
hipError_t launch_mx8_sum(const int8_t* const* q, const uint8_t* const* e, const float* w, int D, uint64_t idx0, int64_t n,
                          const void* ref, fa_dtype rdt, void* out, fa_dtype odt, const Tuning& tu, hipStream_t s);
// Rules 1-3 on the host (fa_mx8_sum_host): plain loops, client by client.
void mx8_sum_host(const int8_t* const* q, const uint8_t* const* e, const float* w, int D, size_t n, uint64_t idx0,
                  const float* ref, float* out);
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
// Top-k receipts (fa.h "Top-k receipts"), fa_topk.hip.  Expansion: dst[i] (dtype ddt, one rounding) := fl(widen(ref[i]) +
// d_i), or d_i without a reference (ref null), over n elements, d_i = val[j] where idx[j] == idx0 + i among the k
// entries and +0 elsewhere; entries outside [idx0, idx0 + n) are skipped, each is range-checked where it is applied.
// Selection over n elements of dtype dt (rules 1-6): idx, val := the min(k, n) entries of fl(widen(y) - widen(sent)), out
// (nullable; y or sent exactly, or apart) := g'; work: topk_workspace(n) bytes, 16-byte aligned, not initialised.
// Any pointers of element alignment: topk_split (host-only) is the split both take, led by dst / by y.
constexpr int kTopkTileElems = 4096;  // the elements of a workgroup's tile, in both directions
Split topk_split(const void* lead, size_t elem, size_t n);
size_t topk_workspace(size_t n);
hipError_t launch_topk_expand(const uint32_t* idx, const float* val, uint64_t k, uint64_t idx0, int64_t n, const void* ref,
                              fa_dtype rdt, void* dst, fa_dtype ddt, hipStream_t s);
hipError_t launch_topk_encode(const void* y, const void* sent, fa_dtype dt, int64_t n, uint64_t k, uint32_t* idx,
                              float* val, void* out, void* work, hipStream_t s);
// Rules 2-5 on the host (fa_topk_encode): the kp <= n entries of the n deltas.
void topk_encode_host(const float* delta, size_t n, size_t kp, uint32_t* idx, float* val);
// Low-rank receipts (fa.h "Low-rank receipts"), fa_lowrank.hip.  The host side: lowrank_check names the first entry
// that breaks the table rules (null: none; *bad its index), the others take a checked table.  lowrank_plan_build
// writes lowrank_plan_bytes bytes: the plan of one launch over bucket elements [idx0, idx0 + cnt).  Expansion: dst[i]
// (dtype ddt, one rounding) := fl(widen(ref[i]) + d_i), or d_i with ref null, over cnt elements from the whole receipt f
// of rank r and the plan of exactly that range, both in device memory; every store is checked against [0, cnt).
const char* lowrank_check(const fa_lowrank_mat* mats, size_t M, uint64_t n, size_t* bad);
uint64_t lowrank_len(const fa_lowrank_mat* mats, size_t M, uint64_t n, int r);
size_t lowrank_plan_bytes(const fa_lowrank_mat* mats, size_t M, uint64_t n, uint64_t idx0, uint64_t cnt);
void lowrank_plan_build(const fa_lowrank_mat* mats, size_t M, uint64_t n, uint64_t idx0, uint64_t cnt, void* plan);
void lowrank_decode_host(const fa_lowrank_mat* mats, size_t M, uint64_t n, const float* f, int r, uint64_t idx0,
                         uint64_t cnt, float* d);
hipError_t launch_lowrank_expand(const void* plan, size_t plan_bytes, const float* f, int r, uint64_t idx0, int64_t cnt,
                                 const void* ref, fa_dtype rdt, void* dst, fa_dtype ddt, hipStream_t s);
// The low-rank-sum stage (fa.h "Low-rank-sum stage"), fa_lowrank_sum.hip.  out[i] (dtype odt, one rounding) :=
// fl32(widen(ref[i]) + acc_i), or acc_i with ref null, over cnt elements from the D whole receipts f[c] of rank r[c]
// (device memory; the arrays f, r and w are host memory) under w[c] and the plan of exactly that range (device
// memory, lowrank_plan_build); every store is checked against [0, cnt).  On a matrix acc_i is the stacked product of
// rules 1-2, elsewhere the fmaf chain of rule 3.
hipError_t launch_lowrank_sum(const void* plan, size_t plan_bytes, const float* const* f, const int* r, const float* w, int D,
                              uint64_t idx0, int64_t cnt, const void* ref, fa_dtype rdt, void* out, fa_dtype odt, hipStream_t s);
// Rules 1-4 on the host (fa_lowrank_sum_host): ascending (c, t) on a matrix, ascending c elsewhere.
void lowrank_sum_host(const fa_lowrank_mat* mats, size_t M, uint64_t n, const float* const* f, const int* r, const float* w,
                      int D, uint64_t idx0, uint64_t cnt, const float* ref, float* out);
// Rot1 receipts (fa.h "Rot1 receipts"), fa_rot1.hip.  Expansion: dst[i] (dtype ddt, one rounding) := fl(widen(ref[i]) +
// d_i), or d_i with ref null, over bucket elements [idx0, idx0 + cnt), any idx0; bits (128 words per block) and scale
// (one per block) start at block idx0 >> 12; every store is checked against the range.  Encoding over n elements of
// dtype dt from block blk0 on (rules 1-6): bits, scale := the codes of fl(widen(y) - widen(sent)), out (nullable; y or
// sent exactly, or apart) := g'.  Any pointers of element alignment.
constexpr int kRot1Block = 4096, kRot1Words = kRot1Block / 32;
hipError_t launch_rot1_expand(const uint32_t* bits, const float* scale, uint64_t seed, uint64_t idx0, int64_t cnt,
                              const void* ref, fa_dtype rdt, void* dst, fa_dtype ddt, hipStream_t s);
hipError_t launch_rot1_encode(const void* y, const void* sent, fa_dtype dt, int64_t n, uint64_t blk0, uint64_t seed,
                              uint32_t* bits, float* scale, void* out, hipStream_t s);
// The codec on the host (fa_rot1_encode, fa_rot1_decode): plain loops over the rule.
void rot1_encode_host(const float* delta, size_t n, uint64_t seed, uint32_t* bits, float* scale);
void rot1_decode_host(const uint32_t* bits, const float* scale, uint64_t seed, uint64_t idx0, size_t cnt, float* d);
// The rot1-sum stage (fa.h "Rot1-sum stage"), fa_rot1_sum.hip.  out[i] (dtype odt, one rounding) := fl32(widen(ref[i]) +
// acc_i), or acc_i with ref null, over bucket elements [idx0, idx0 + cnt), any idx0, from the D receipts (bits[c], scale[c],
// seed[c]) under w[c]; bits[c] (128 words per block) and scale[c] (one per block) start at block idx0 >> 12 (device memory;
// the arrays bits, scale, seed and w are host memory); a block the range holds part of is reduced whole and every store
// is checked against the range.  (rdt, odt) as dtype_pair_ok(in, out); out may be ref exactly (a lane reads its elements
// before it writes them).  rot1_sum_vec (host-only): whether a lane's 16 elements move in 16-byte accesses.
constexpr int kRot1SumDepth = 8;  // the owners whose half-words a lane keeps in flight
bool rot1_sum_vec(uint64_t idx0, const void* ref, fa_dtype rdt, const void* out, fa_dtype odt);
hipError_t launch_rot1_sum(const uint32_t* const* bits, const float* const* scale, const uint64_t* seed, const float* w, int D,
                           uint64_t idx0, int64_t cnt, const void* ref, fa_dtype rdt, void* out, fa_dtype odt, const Tuning& tu,
                           hipStream_t s);
// Rule 0: order[k] is the owner at place k, first[k] whether place k starts a group.
void rot1_sum_order(const uint64_t* seed, int D, int* order, uint8_t* first);
// Rules 0-6 on the host (fa_rot1_sum_host): plain loops, block by block and group by group.
void rot1_sum_host(const uint32_t* const* bits, const float* const* scale, const uint64_t* seed, const float* w, int D,
                   uint64_t idx0, size_t cnt, const float* ref, float* out);
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
