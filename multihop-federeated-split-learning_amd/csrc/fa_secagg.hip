// fa_secagg.hip -- the secagg stage (fa.h "Secagg stage") for CDNA4 (gfx950): u_i = sum_k y_{k,i} + sum_t sign_t m_{t,i}
// modulo 2^32 over D buckets of uint32 words and T ChaCha20 mask streams, then a_i = fl32((float)(int32_t)u_i * scale).
//
// The term loop is the whole cost: a ChaCha20 block is 20 rounds of 4 quarter-rounds of 4 adds, 4 xors and 4 rotations
// (one v_alignbit_b32 each), 960 VALU instructions for 16 elements of one term, against 4 bytes read per element and
// client.  Nothing of it touches memory: key and nonce are wave-uniform, read from the term table with scalar loads
// (the table pointer is cast to the constant address space, so the loads stay scalar beside the kernel's stores).
//
// What the host takes out of the loop (secagg_table).  The block function ends by adding the initial state to the
// working state.  That addition commutes with the signed sum over the terms, and the initial state is wave-uniform
// but for the counter: the table starts with U_j = sum_t sign_t init_{t,j} for the 15 uniform words (constants, key,
// nonce), and the counter word gets (P - N) ctr with P and N the counts of the two signs.  The terms are stored with
// the +1 terms first, so the sign is a loop bound, not a per-word negation.  A term then costs the 960 round
// instructions and 16 accumulations.
//
// Tile and registers.  A tile is 64 blocks = 1024 consecutive bucket elements starting at a multiple of 16 of the
// bucket index; lane l owns block j0 + l: 16 working words, 16 uint32 accumulators, the counter (registers and
// occupancy: DESIGN.md 8j).  After the loop a lane holds 64 contiguous bytes of mask sum, while the D bucket loads want
// 16-byte vectors with vector l + 64 r on lane l.  The sums cross a wave-private LDS tile once per tile: lane l writes
// its four quarters into row l (4 ds_write_b128), rows kRowWords = 20 dwords apart, and reads vector v = l + 64 r from
// row v >> 2, quarter v & 3 (4 ds_read_b128).  Bank conflicts, counted from the addresses for 64 banks and 16 lanes per
// pass of a 128-bit access: a write pass touches dwords 20 l + 4 q + (0..3), l = 16 consecutive lanes -- 20 l mod 64
// takes 16 different multiples of 4, no conflict (unpadded rows of 16 dwords would put lanes l and l + 4 on the same
// banks, 4 ways); a read pass touches rows 4 p .. 4 p + 3 at every quarter, dwords 20 b + 4 q: the fourth row wraps
// onto the first row's banks in 3 of its 4 quarters, so 3 of 16 lanes wait one more cycle.  Not measured.
//
// Two forms of the vector path, the same bits (modular addition is associative):
//   tile per wave   every wave of the grid walks tiles of its own; no workgroup barrier.
//   term split      the four waves of a workgroup share a tile: wave w expands terms [w T/4, (w+1) T/4), writes its
//                   partial sums into its LDS tile, and after one barrier takes vectors l + 64 w: the four partial
//                   sums from LDS, U from the table, then its share of the loads and stores.  For buckets with fewer
//                   tiles than the chip has SIMDs (secagg_form).
// The element form (one element per lane, its whole block per term, one word kept) runs the head before the first
// tile, the tail after the last whole vector, and a launch whose pointer phase and bucket-index phase disagree
// modulo 4 (secagg_split).  D beyond kMaxClients: earlier passes store the uint32 sums (OUT = uint32_t, no terms), the
// last one continues them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fa_device.h"
#include "fa_internal.h"

#pragma clang fp contract(off)

namespace fa {

namespace {

constexpr int kTabTerms = 16;   // the table: U_0 .. U_15 (U_12 = 0), then kTermWords words per term
constexpr int kTermWords = 12;  // key (8), nonce (3), one word of padding: a term is three 16-byte scalar loads
constexpr int kRowWords = 20;   // LDS row of a block's 16 words, padded (above)
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int64_t kTileVecs = 256;  // 64 blocks of 4 vectors

#define FA_QR(a, b, c, d)               \
    a += b; d ^= a; d = __builtin_rotateleft32(d, 16); \
    c += d; b ^= c; b = __builtin_rotateleft32(b, 12); \
    a += b; d ^= a; d = __builtin_rotateleft32(d, 8);  \
    c += d; b ^= c; b = __builtin_rotateleft32(b, 7);

// The 20 rounds of RFC 8439 2.3 on the state x, without the final addition.
__host__ __device__ __forceinline__ void chacha_rounds(uint32_t* x) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        FA_QR(x[0], x[4], x[8], x[12])
        FA_QR(x[1], x[5], x[9], x[13])
        FA_QR(x[2], x[6], x[10], x[14])
        FA_QR(x[3], x[7], x[11], x[15])
        FA_QR(x[0], x[5], x[10], x[15])
        FA_QR(x[1], x[6], x[11], x[12])
        FA_QR(x[2], x[7], x[8], x[13])
        FA_QR(x[3], x[4], x[9], x[14])
    }
}
#undef FA_QR

// "expand 32-byte k"
constexpr uint32_t sigma(int j) { return j == 0 ? 0x61707865u : j == 1 ? 0x3320646eu : j == 2 ? 0x79622d32u : 0x6b206574u; }

typedef const __attribute__((address_space(4))) uint32_t* ConstWords;

struct SecaggArgs {
    const uint32_t* tab;   // device: the term table (null with T == 0)
    const uint32_t* init;  // nullable: the uint32 sums of the earlier passes
    void* out;
    float scale;
    int nc, T, npos;
    uint32_t cnet;  // P - N modulo 2^32
    int64_t head, nvec, ntile;
    uint64_t blk0;  // the block of the first tile: (idx0 + head) >> 4
};

// acc += the signed working states of terms [t0, t1) at block counter ctr (the +1 terms are [0, npos)).
__device__ __forceinline__ void expand_terms(ConstWords tab, int t0, int t1, int npos, uint32_t ctr, uint32_t* acc) {
#pragma clang loop unroll(disable)
    for (int t = t0; t < t1; ++t) {
        ConstWords k = tab + kTabTerms + t * kTermWords;
        uint32_t x[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = sigma(j);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[4 + j] = k[j];
        x[12] = ctr;
#pragma unroll
        for (int j = 0; j < 3; ++j) x[13 + j] = k[8 + j];
        chacha_rounds(x);
        if (t < npos) {  // wave-uniform
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += x[j];
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] -= x[j];
        }
    }
}

// LDS traffic of one wave with itself: the compiler may not move accesses across, the hardware keeps a wave's DS
// operations in order.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float decode(uint32_t u, float scale) {
#pragma clang fp contract(off)
    const float f = (float)(int32_t)u;  // v_cvt_f32_i32: to nearest-even
    return f * scale;
}

// R vectors of a tile per lane, vector v0 + 64 r with mask sum m[r]: + init, + the nc buckets, decode, store.  A lane
// whose vector lies past the bucket loads the last one instead and stores nothing.
template <typename OUT, int SP, int R>
__device__ __forceinline__ void finish_vecs(const ClientTable& ct, const SecaggArgs& a, int64_t v0, u32x4* m) {
    int64_t e[R];
    bool ok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t v = v0 + 64 * r;
        ok[r] = v < a.nvec;
        e[r] = a.head + 4 * (ok[r] ? v : a.nvec - 1);
        if (a.init) m[r] += ld16<false>(a.init + e[r]);
    }
    constexpr int G = 16 / R;  // loads in flight per lane: 16
    int k = 0;
    for (; k + G <= a.nc; k += G) {
        u32x4 x[G][R];
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r) x[j][r] = ld16<true>(static_cast<const uint32_t*>(ct.src[k + j]) + e[r]);
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r) m[r] += x[j][r];
    }
    for (; k < a.nc; ++k)
#pragma unroll
        for (int r = 0; r < R; ++r) m[r] += ld16<true>(static_cast<const uint32_t*>(ct.src[k]) + e[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!ok[r]) continue;
        if constexpr (sizeof(OUT) == 4 && !__is_same(OUT, float)) {  // uint32_t: the sums as they are
            st16<SP>(static_cast<uint32_t*>(a.out) + e[r], m[r]);
        } else {
            const float f[4] = {decode(m[r].x, a.scale), decode(m[r].y, a.scale), decode(m[r].z, a.scale),
                                decode(m[r].w, a.scale)};
            Out<OUT>::template store<4, SP>(a.out, e[r], f);
        }
    }
}

// Tile per wave.
template <typename OUT, int SP>
__global__ __launch_bounds__(kThreads) void secagg_tile_kernel(const ClientTable ct, const SecaggArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][64 * kRowWords];
    const int lane = (int)(threadIdx.x & 63u);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* my = lds[w];
    ConstWords tab = (ConstWords)a.tab;
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + w; tile < a.ntile; tile += waves) {
        u32x4 m[4] = {u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}};
        if (a.T > 0) {  // wave-uniform
            const uint32_t ctr = (uint32_t)(a.blk0 + (uint64_t)tile * 64u + (uint64_t)lane);
            uint32_t acc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = tab[j];
            acc[12] = a.cnet * ctr;
            expand_terms(tab, 0, a.T, a.npos, ctr, acc);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<u32x4*>(my + lane * kRowWords + 4 * q) =
                    u32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
            wave_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r)
                m[r] = *reinterpret_cast<const u32x4*>(my + ((lane >> 2) + 16 * r) * kRowWords + 4 * (lane & 3));
            wave_sync();  // the next tile's writes follow these reads
        }
        finish_vecs<OUT, SP, 4>(ct, a, tile * kTileVecs + lane, m);
    }
}

// Term split: one tile per workgroup and trip, T > 0.
template <typename OUT, int SP>
__global__ __launch_bounds__(kThreads) void secagg_split_kernel(const ClientTable ct, const SecaggArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][64 * kRowWords];
    const int lane = (int)(threadIdx.x & 63u);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    ConstWords tab = (ConstWords)a.tab;
    const int per = (a.T + kWaves - 1) / kWaves;
    const int t0 = min(a.T, w * per), t1 = min(a.T, t0 + per);
    for (int64_t tile = (int64_t)blockIdx.x; tile < a.ntile; tile += (int64_t)gridDim.x) {  // uniform over the workgroup
        const uint64_t blk = a.blk0 + (uint64_t)tile * 64u;
        uint32_t acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0u;
        expand_terms(tab, t0, t1, a.npos, (uint32_t)(blk + (uint64_t)lane), acc);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<u32x4*>(lds[w] + lane * kRowWords + 4 * q) =
                u32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        __syncthreads();
        const int b = (lane >> 2) + 16 * w, q = lane & 3;  // vector lane + 64 w: quarter q of block b
        u32x4 m = ld16<false>(a.tab + 4 * q);              // U of the quarter; the counter word's share below
        if (q == 3) m.x += a.cnet * (uint32_t)(blk + (uint64_t)b);
#pragma unroll
        for (int o = 0; o < kWaves; ++o) m += *reinterpret_cast<const u32x4*>(lds[o] + b * kRowWords + 4 * q);
        finish_vecs<OUT, SP, 1>(ct, a, tile * kTileVecs + lane + 64 * w, &m);
        __syncthreads();  // the next tile's writes follow these reads
    }
}

// Element form over elements [0, head) and [tail0, n) (the whole range: head = tail0 = n), one per lane and trip.
template <typename OUT>
__global__ __launch_bounds__(kThreads) void secagg_elem_kernel(const ClientTable ct, const SecaggArgs a, int64_t head,
                                                               int64_t tail0, int64_t n, uint64_t idx0) {
    ConstWords tab = (ConstWords)a.tab;
    const int64_t cnt = head + (n - tail0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cnt; s += stride) {
        const int64_t i = s < head ? s : tail0 + (s - head);
        const uint64_t g = idx0 + (uint64_t)i;
        const uint32_t ctr = (uint32_t)(g >> 4), word = (uint32_t)g & 15u;
        uint32_t sum = 0u;
        if (a.T > 0) {
            uint32_t acc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = tab[j];
            acc[12] = a.cnet * ctr;
            expand_terms(tab, 0, a.T, a.npos, ctr, acc);
            sum = acc[0];
#pragma unroll
            for (int j = 1; j < 16; ++j) sum = word == (uint32_t)j ? acc[j] : sum;
        }
        if (a.init) sum += a.init[i];
        for (int k = 0; k < a.nc; ++k) sum += static_cast<const uint32_t*>(ct.src[k])[i];
        if constexpr (sizeof(OUT) == 4 && !__is_same(OUT, float)) static_cast<uint32_t*>(a.out)[i] = sum;
        else Out<OUT>::scalar(a.out, i, decode(sum, a.scale));
    }
}

// The rule of secagg_form, in one place: the term split is for buckets with fewer tiles than 256 CUs have SIMDs --
// a tile per wave leaves SIMDs idle there -- once every wave of a workgroup gets at least kSplitMinTerms / 4 terms,
// enough to pay for the barrier and the four-fold LDS read.
constexpr int64_t kSplitMaxTiles = 256 * 4;
constexpr int kSplitMinTerms = 16;
constexpr int64_t kMaxBlocks = 2048;        // 8 workgroups of 20 KiB LDS per CU on 256 CUs; tiles beyond it are strided
constexpr int64_t kElemMaxBlocks = 1 << 16;

template <typename OUT>
hipError_t launch_secagg_t(const ClientTable& ct, SecaggArgs a, uint64_t idx0, const Split& sp, int form,
                           const Tuning& tu, hipStream_t s) {
    const int64_t cap = tu.max_blocks > 0 ? std::min<int64_t>(kMaxBlocks, tu.max_blocks) : kMaxBlocks;
    if (sp.vec && sp.nvec > 0) {
        a.head = sp.head;
        a.nvec = sp.nvec;
        a.ntile = (sp.nvec + kTileVecs - 1) / kTileVecs;
        a.blk0 = (idx0 + (uint64_t)sp.head) >> 4;
        if (form == kSecaggSplit && a.T > 0)
            hipLaunchKernelGGL((secagg_split_kernel<OUT, kStSc1>), dim3((unsigned)std::min(a.ntile, cap)), dim3(kThreads), 0,
                               s, ct, a);
        else
            hipLaunchKernelGGL((secagg_tile_kernel<OUT, kStSc1>),
                               dim3((unsigned)std::min((a.ntile + kWaves - 1) / kWaves, cap)), dim3(kThreads), 0, s, ct, a);
        if (sp.edges() > 0)
            hipLaunchKernelGGL((secagg_elem_kernel<OUT>), dim3(1), dim3(64), 0, s, ct, a, sp.head, sp.tail0(), sp.n, idx0);
        return hipGetLastError();
    }
    const int64_t blocks = std::max<int64_t>(1, std::min((sp.n + kThreads - 1) / kThreads, std::min(cap * 32, kElemMaxBlocks)));
    hipLaunchKernelGGL((secagg_elem_kernel<OUT>), dim3((unsigned)blocks), dim3(kThreads), 0, s, ct, a, sp.n, sp.n, sp.n, idx0);
    return hipGetLastError();
}

}  // namespace

int secagg_form(int64_t n, int T) {
    const int64_t tiles = (n + 4 * kTileVecs - 1) / (4 * kTileVecs);
    return T >= kSplitMinTerms && tiles < kSplitMaxTiles ? kSecaggSplit : kSecaggTile;
}

Split secagg_split(const void* lead, uint64_t idx0, size_t n) {
    Split sp = split_at(lead, 4, n);
    if (((idx0 + (uint64_t)sp.lead) & 3u) != 0) {  // no head brings the pointer to 16 bytes and the index to a block
        sp.vec = false;
        return sp;
    }
    const int64_t lead16 = (int64_t)((16u - (idx0 & 15u)) & 15u);  // = sp.lead modulo 4
    const int64_t head = lead16 < (int64_t)n ? lead16 : (int64_t)n;
    return Split{head, ((int64_t)n - head) / 4, (int64_t)n, 4, lead16, true};
}

void secagg_table(int T, const uint32_t* keys, const uint32_t* nonces, const int* signs, uint32_t* tab, int* npos,
                  uint32_t* cnet) {
    int P = 0;
    for (int t = 0; t < T; ++t) P += signs[t] > 0;
    for (int j = 0; j < kTabTerms; ++j) tab[j] = 0u;
    int at[2] = {0, P};  // where the next +1 and the next -1 term go
    for (int t = 0; t < T; ++t) {
        const bool neg = signs[t] < 0;
        uint32_t* k = tab + kTabTerms + (size_t)at[neg]++ * kTermWords;
        for (int j = 0; j < 8; ++j) k[j] = keys[(size_t)t * 8 + j];
        for (int j = 0; j < 3; ++j) k[8 + j] = nonces[(size_t)t * 3 + j];
        k[11] = 0u;
        for (int j = 0; j < 8; ++j) tab[4 + j] += neg ? 0u - k[j] : k[j];
        for (int j = 0; j < 3; ++j) tab[13 + j] += neg ? 0u - k[8 + j] : k[8 + j];
    }
    const uint32_t net = (uint32_t)P - (uint32_t)(T - P);
    for (int j = 0; j < 4; ++j) tab[j] = net * sigma(j);
    *npos = P;
    *cnet = net;
}

size_t secagg_table_words(int T) { return (size_t)kTabTerms + (size_t)T * kTermWords; }

hipError_t launch_secagg(const ClientTable& t, int nc, const uint32_t* tab, int T, int npos, uint32_t cnet,
                         const uint32_t* init, void* out, fa_dtype odt, bool raw, float scale, uint64_t idx0,
                         const Split& sp, int form, const Tuning& tu, hipStream_t s) {
    if (sp.n <= 0) return hipSuccess;
    if (!sp.valid() || sp.V != 4 || !out || nc < 0 || nc > kMaxClients || T < 0 || (T > 0 && !tab)) return hipErrorInvalidValue;
    if (sp.vec && ((idx0 + (uint64_t)sp.head) & 15u) != 0 && sp.nvec > 0) return hipErrorInvalidValue;
    if (form != kSecaggTile && form != kSecaggSplit) form = secagg_form(sp.n, T);
    SecaggArgs a{tab, init, out, scale, nc, raw ? 0 : T, npos, cnet, 0, 0, 0, 0};
    if (raw) return launch_secagg_t<uint32_t>(t, a, idx0, sp, form, tu, s);
    switch (odt) {
        case FA_F32: return launch_secagg_t<float>(t, a, idx0, sp, form, tu, s);
        case FA_BF16: return launch_secagg_t<uint16_t>(t, a, idx0, sp, form, tu, s);
        case FA_F16: return launch_secagg_t<_Float16>(t, a, idx0, sp, form, tu, s);
    }
    return hipErrorInvalidValue;
}

void secagg_mask_host(const uint32_t* key, const uint32_t* nonce, uint64_t idx0, size_t n, uint32_t* out) {
    size_t done = 0;
    while (done < n) {
        const uint64_t g = idx0 + done;
        uint32_t init[16], x[16];
        for (int j = 0; j < 4; ++j) init[j] = sigma(j);
        for (int j = 0; j < 8; ++j) init[4 + j] = key[j];
        init[12] = (uint32_t)(g >> 4);
        for (int j = 0; j < 3; ++j) init[13 + j] = nonce[j];
        for (int j = 0; j < 16; ++j) x[j] = init[j];
        chacha_rounds(x);
        for (uint32_t j = (uint32_t)g & 15u; j < 16 && done < n; ++j) out[done++] = x[j] + init[j];
    }
}

}  // namespace fa
