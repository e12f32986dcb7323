// albedo.hip — the albedo evaluation of the TensoIR protocol (the reference's albedo_eval.py) on the device, where the albedo frames already are:
//   mirres_albedo_compact   masked compaction of one view's (prediction, ground truth) pairs into a pool, in pixel order (albedo_eval.py:93-111);
//   mirres_albedo_median    channel-wise EXACT median of double(gt) / max(double(pred), 1e-6) over the pool, numpy's definition (:116-118);
//   mirres_albedo_score     one view's aligned squared-error sums (linear and gamma 2.2) in fp64 and the two 8-bit gamma images (:142-172).
// Every result is a function of the inputs alone: counts and the selected keys travel through integer atomics, floating-point sums through fixed trees.
// The median is a radix select over an order-preserving 64-bit key of the ratio, recomputed from the fp32 pair in every pass (24 B per pixel and
// pass; storing the keys would cost as much to write once and to read back in every pass): 8 passes of 8-bit digits, per-workgroup LDS histograms
// flushed by integer atomics, the bucket of the wanted rank found by a one-workgroup kernel between the passes (no host round trip); for an even
// count one more pass counts the values <= v_k and finds the smallest one above it (DESIGN.md §5 "Albedo evaluation").
#include <algorithm>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_scan.hpp"

namespace mr {

#define AL_BLOCK 256
#define AL_PARTS 1024        // contiguous pixel segments of the compaction and of the score, one workgroup each: the order of every append / sum is fixed by n alone
#define AL_GRID 2048         // workgroups of a select pass (grid stride over groups of 4 pixels)
#define AL_BINS 256
#define AL_NANKEY 0xFFFFFFFFFFFFFFFFULL   // every NaN ratio: above +inf, so the order of the other keys is untouched

typedef unsigned long long u64;

// per-channel select state, in the caller's scratch
struct AlSel {
    u64 hist[AL_BINS];
    u64 prefix;      // digits of the rank-k key found so far (high bits)
    u64 rank;        // rank of the wanted key among the keys that share the prefix
    u64 nan;         // NaN ratios in the pool
    u64 le;          // even counts: keys <= the rank-k key
    u64 above;       // even counts: smallest key above it
    u64 pad[3];
};
struct AlScratch { AlSel sel[3]; };
static_assert(sizeof(AlScratch) <= MIRRES_ALBEDO_SCRATCH_BYTES, "albedo scratch");
static_assert(sizeof(u64) * (AL_PARTS + 1) <= MIRRES_ALBEDO_SCRATCH_BYTES && sizeof(double) * 2 * AL_PARTS <= MIRRES_ALBEDO_SCRATCH_BYTES, "albedo scratch");

// albedo_eval.py:117 for one channel: gt / pred.clip(min=1e-6) in float64 (np.clip keeps a NaN prediction: the comparison is false for it),
// as a key whose unsigned order is the order of the values: negative values with all bits flipped, the others with the sign bit set.
MR_DEV u64 ratio_key(float pred, float gt) {
    double p = (double)pred;
    if (p < 1e-6) p = 1e-6;
    const double r = (double)gt / p;
    if (r != r) return AL_NANKEY;
    const u64 b = (u64)__double_as_longlong(r);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
MR_DEV double key_value(u64 k) {
    const u64 b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
    return __longlong_as_double((long long)b);
}

// ------------------------------------------------------------------------------------------------ (a) masked compaction
MR_DEV bool kept(const float* __restrict__ gt_rgba, long long i, double thr) { return (double)gt_rgba[4 * i + 3] >= thr; }   // :94-95 clears the mask where alpha < thr

__global__ void __launch_bounds__(AL_BLOCK) k_compact_count(const float* __restrict__ gt_rgba, long long n, long long seg, double thr, u64* __restrict__ counts,
                                                            u64* __restrict__ state) {
    __shared__ unsigned int sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0;
    __syncthreads();
    const long long i0 = (long long)blockIdx.x * seg, i1 = min(n, i0 + seg);
    unsigned int c = 0, bad = 0;
    for (long long i = i0 + threadIdx.x; i < i1; i += AL_BLOCK) {
        if (!kept(gt_rgba, i, thr)) continue;
        c++;
        if (gt_rgba[4 * i] > 1.f || gt_rgba[4 * i + 1] > 1.f || gt_rgba[4 * i + 2] > 1.f) bad++;      // :98-100
    }
    if (c) atomicAdd(&sh[0], c);
    if (bad) atomicAdd(&sh[1], bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = sh[0];
        if (sh[1]) atomicAdd(&state[1], (u64)sh[1]);
    }
}

// exclusive scan (block_excl_scan, device_scan.hpp) of the AL_PARTS segment counts, offset by the pool's count, which then grows by the total (clamped to the capacity: state[2] reports the overflow)
__global__ void __launch_bounds__(AL_BLOCK) k_compact_scan(u64* __restrict__ counts, u64* __restrict__ state, u64 cap) {
    __shared__ u64 sh[AL_BLOCK / 64];
    constexpr int PER = AL_PARTS / AL_BLOCK;
    u64 v[PER], s = 0, all;
    for (int k = 0; k < PER; k++) { v[k] = counts[PER * threadIdx.x + k]; s += v[k]; }
    const u64 excl = block_excl_scan<AL_BLOCK>(s, sh, all);
    const u64 base = state[0];                              // every thread reads it before the barrier below, one writes it after
    u64 run = base + excl;
    for (int k = 0; k < PER; k++) { counts[PER * threadIdx.x + k] = run; run += v[k]; }
    __syncthreads();
    if (threadIdx.x == AL_BLOCK - 1) {
        const u64 total = base + all;
        if (total > cap) state[2] = 1;
        state[0] = total > cap ? cap : total;
    }
}

__global__ void __launch_bounds__(AL_BLOCK) k_compact_scatter(const float* __restrict__ pred, const float* __restrict__ gt_rgba, long long n, long long seg, double thr,
                                                              const u64* __restrict__ offsets, float* __restrict__ pool_pred, float* __restrict__ pool_gt, u64 cap) {
    __shared__ unsigned int wave_n[AL_BLOCK / 64];
    const long long i0 = (long long)blockIdx.x * seg, i1 = min(n, i0 + seg);
    u64 run = offsets[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long t0 = i0; t0 < i1; t0 += AL_BLOCK) {          // uniform trip count: every thread reaches the barriers
        const long long i = t0 + threadIdx.x;
        const bool k = i < i1 && kept(gt_rgba, i, thr);
        const u64 m = __ballot(k);
        if (lane == 0) wave_n[wave] = (unsigned int)__popcll(m);
        __syncthreads();
        u64 before = 0, all = 0;
        for (int w = 0; w < AL_BLOCK / 64; w++) { if (w < wave) before += wave_n[w]; all += wave_n[w]; }
        const u64 dst = run + before + (u64)__popcll(m & ((1ULL << lane) - 1ULL));
        if (k && dst < cap) {
            for (int c = 0; c < 3; c++) { pool_pred[3 * dst + c] = pred[3 * i + c]; pool_gt[3 * dst + c] = gt_rgba[4 * i + c]; }
        }
        run += all;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ (b) exact median: radix select
__global__ void k_select_init(AlScratch* __restrict__ sc, u64 rank) {
    for (int c = 0; c < 3; c++) {
        for (int i = threadIdx.x; i < AL_BINS; i += blockDim.x) sc->sel[c].hist[i] = 0;
        if (threadIdx.x == 0) { AlSel& s = sc->sel[c]; s.prefix = 0; s.rank = rank; s.nan = 0; s.le = 0; s.above = AL_NANKEY; }
    }
}

// the 12 predictions and 12 ground-truth values of pixels 4g .. 4g + 3 (three 16-byte loads per pool when the whole group exists)
MR_DEV int load_group(const float* __restrict__ pool_pred, const float* __restrict__ pool_gt, u64 g, u64 n, float* p, float* q) {
    const u64 i = 4 * g;
    if (i + 4 <= n) {
        const float4* a = reinterpret_cast<const float4*>(pool_pred + 3 * i);
        const float4* b = reinterpret_cast<const float4*>(pool_gt + 3 * i);
        for (int k = 0; k < 3; k++) {
            const float4 x = a[k], y = b[k];
            p[4 * k] = x.x; p[4 * k + 1] = x.y; p[4 * k + 2] = x.z; p[4 * k + 3] = x.w;
            q[4 * k] = y.x; q[4 * k + 1] = y.y; q[4 * k + 2] = y.z; q[4 * k + 3] = y.w;
        }
        return 4;
    }
    const int m = (int)(n - i);
    for (int k = 0; k < 3 * m; k++) { p[k] = pool_pred[3 * i + k]; q[k] = pool_gt[3 * i + k]; }
    return m;
}

// histogram of the digit at `shift` over the keys that carry the prefix found so far. A thread keeps (bin, count) per channel while consecutive keys fall into
// one bin — neighbouring pixels mostly share sign and exponent, i.e. the leading digits — and goes to the LDS atomic only when the bin changes.
__global__ void __launch_bounds__(AL_BLOCK) k_select_hist(const float* __restrict__ pool_pred, const float* __restrict__ pool_gt, u64 n, int shift, AlScratch* __restrict__ sc) {
    __shared__ unsigned int lh[3][AL_BINS];
    __shared__ unsigned int lnan[3];
    for (int i = threadIdx.x; i < 3 * AL_BINS; i += AL_BLOCK) (&lh[0][0])[i] = 0;
    if (threadIdx.x < 3) lnan[threadIdx.x] = 0;
    __syncthreads();
    u64 prefix[3];
    for (int c = 0; c < 3; c++) prefix[c] = sc->sel[c].prefix;
    const bool first = shift == 56;
    int bin[3] = {0, 0, 0};
    unsigned int cnt[3] = {0, 0, 0}, nan[3] = {0, 0, 0};
    const u64 groups = (n + 3) / 4;                             // n < 2^40 (entry point): a workgroup sees fewer than 2^32 keys
    for (u64 g = (u64)blockIdx.x * AL_BLOCK + threadIdx.x; g < groups; g += (u64)AL_GRID * AL_BLOCK) {
        float p[12], q[12];
        const int m = load_group(pool_pred, pool_gt, g, n, p, q);
        for (int j = 0; j < m; j++)
            for (int c = 0; c < 3; c++) {
                const u64 key = ratio_key(p[3 * j + c], q[3 * j + c]);
                if (first) { if (key == AL_NANKEY) nan[c]++; }
                else if ((key >> (shift + 8)) != (prefix[c] >> (shift + 8))) continue;
                const int b = (int)((key >> shift) & (AL_BINS - 1));
                if (b != bin[c]) { if (cnt[c]) atomicAdd(&lh[c][bin[c]], cnt[c]); bin[c] = b; cnt[c] = 0; }
                cnt[c]++;
            }
    }
    for (int c = 0; c < 3; c++) {
        if (cnt[c]) atomicAdd(&lh[c][bin[c]], cnt[c]);
        if (nan[c]) atomicAdd(&lnan[c], nan[c]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * AL_BINS; i += AL_BLOCK) {
        const unsigned int v = (&lh[0][0])[i];
        if (v) atomicAdd(&sc->sel[i / AL_BINS].hist[i % AL_BINS], (u64)v);
    }
    if (threadIdx.x < 3 && lnan[threadIdx.x]) atomicAdd(&sc->sel[threadIdx.x].nan, (u64)lnan[threadIdx.x]);
}

// the bin that holds the wanted rank: its digit joins the prefix, the rank becomes the rank inside the bin; the histogram is cleared for the next pass
__global__ void __launch_bounds__(AL_BINS) k_select_pick(AlScratch* __restrict__ sc, int shift) {
    __shared__ u64 h[3][AL_BINS];
    for (int c = 0; c < 3; c++) { h[c][threadIdx.x] = sc->sel[c].hist[threadIdx.x]; sc->sel[c].hist[threadIdx.x] = 0; }
    __syncthreads();
    if (threadIdx.x < 3) {
        AlSel& s = sc->sel[threadIdx.x];
        u64 k = s.rank, cum = 0;
        int b = 0;
        for (; b < AL_BINS - 1; b++) {
            const u64 v = h[threadIdx.x][b];
            if (k < cum + v) break;
            cum += v;
        }
        s.rank = k - cum;
        s.prefix |= (u64)b << shift;
    }
}

// even counts: how many keys are <= the rank-k key, and the smallest key above it
__global__ void __launch_bounds__(AL_BLOCK) k_select_next(const float* __restrict__ pool_pred, const float* __restrict__ pool_gt, u64 n, AlScratch* __restrict__ sc) {
    __shared__ u64 sh_le[3], sh_above[3];
    if (threadIdx.x < 3) { sh_le[threadIdx.x] = 0; sh_above[threadIdx.x] = AL_NANKEY; }
    __syncthreads();
    u64 kk[3], le[3] = {0, 0, 0}, above[3] = {AL_NANKEY, AL_NANKEY, AL_NANKEY};
    for (int c = 0; c < 3; c++) kk[c] = sc->sel[c].prefix;
    const u64 groups = (n + 3) / 4;
    for (u64 g = (u64)blockIdx.x * AL_BLOCK + threadIdx.x; g < groups; g += (u64)AL_GRID * AL_BLOCK) {
        float p[12], q[12];
        const int m = load_group(pool_pred, pool_gt, g, n, p, q);
        for (int j = 0; j < m; j++)
            for (int c = 0; c < 3; c++) {
                const u64 key = ratio_key(p[3 * j + c], q[3 * j + c]);
                if (key <= kk[c]) le[c]++;
                else if (key < above[c]) above[c] = key;
            }
    }
    for (int c = 0; c < 3; c++) {
        if (le[c]) atomicAdd(&sh_le[c], le[c]);
        if (above[c] != AL_NANKEY) atomicMin(&sh_above[c], above[c]);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        if (sh_le[threadIdx.x]) atomicAdd(&sc->sel[threadIdx.x].le, sh_le[threadIdx.x]);
        if (sh_above[threadIdx.x] != AL_NANKEY) atomicMin(&sc->sel[threadIdx.x].above, sh_above[threadIdx.x]);
    }
}

// np.median: the middle value, or for an even count the mean (a + b) / 2 of the two middle ones; NaN as soon as one ratio is NaN
__global__ void k_select_finish(const AlScratch* __restrict__ sc, u64 n, double* __restrict__ out3) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    const AlSel& s = sc->sel[c];
    const double a = key_value(s.prefix);
    double r = a;
    if (!(n & 1)) {
        const u64 k = n / 2 - 1;
        const double b = s.le > k + 1 ? a : key_value(s.above);
        r = (a + b) / 2.0;
    }
    if (s.nan) r = __longlong_as_double(0x7FF8000000000000LL);
    out3[c] = r;
}

// ------------------------------------------------------------------------------------------------ (c) per-view score
MR_DEV double clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }            // np.clip: a NaN stays
MR_DEV uint8_t to_u8(double x) { const double v = x * 255.0; return (uint8_t)(v >= 255.0 ? 255 : (v > 0.0 ? (int)v : 0)); }   // astype('uint8'): truncation

// fixed tree over the workgroup's 256 partial pairs
MR_DEV void block_sum2(double& a, double& b, double (*sh)[2]) {
    sh[threadIdx.x][0] = a; sh[threadIdx.x][1] = b;
    __syncthreads();
    for (int off = AL_BLOCK / 2; off > 0; off >>= 1) {
        if (threadIdx.x < (unsigned)off) { sh[threadIdx.x][0] += sh[threadIdx.x + off][0]; sh[threadIdx.x][1] += sh[threadIdx.x + off][1]; }
        __syncthreads();
    }
    a = sh[0][0]; b = sh[0][1];
}

__global__ void __launch_bounds__(AL_BLOCK) k_score(const float* __restrict__ pred, const float* __restrict__ gt_rgba, long long n, long long seg, double thr,
                                                    double s0, double s1, double s2, double* __restrict__ partial, uint8_t* __restrict__ out_pred, uint8_t* __restrict__ out_gt) {
    __shared__ double sh[AL_BLOCK][2];
    const double scale[3] = {s0, s1, s2};
    const double ig = 1.0 / 2.2;
    const long long i0 = (long long)blockIdx.x * seg, i1 = min(n, i0 + seg);
    double lin = 0.0, gam = 0.0;
    for (long long i = i0 + threadIdx.x; i < i1; i += AL_BLOCK) {
        const bool k = kept(gt_rgba, i, thr);
        for (int c = 0; c < 3; c++) {
            const double now = k ? clip01((double)pred[3 * i + c] * scale[c]) : 1.0;     // :104, :147-149 (the unmasked 1 is its own clip)
            const double gt = k ? (double)gt_rgba[4 * i + c] : 1.0;                      // :103
            const double gn = pow(now, ig), gg = pow(gt, ig);                            // :150-151
            const double dl = gt - now, dg = gg - gn;
            lin += dl * dl; gam += dg * dg;                                              // :166, :170
            if (out_pred) out_pred[3 * i + c] = to_u8(gn);                               // :153-154
            if (out_gt) out_gt[3 * i + c] = to_u8(gg);
        }
    }
    block_sum2(lin, gam, sh);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = lin; partial[2 * blockIdx.x + 1] = gam; }
}

__global__ void __launch_bounds__(AL_BLOCK) k_score_sum(const double* __restrict__ partial, double* __restrict__ out2) {
    __shared__ double sh[AL_BLOCK][2];
    double a = 0.0, b = 0.0;
    for (int k = 0; k < AL_PARTS / AL_BLOCK; k++) { a += partial[2 * (AL_BLOCK * k + threadIdx.x)]; b += partial[2 * (AL_BLOCK * k + threadIdx.x) + 1]; }
    block_sum2(a, b, sh);
    if (threadIdx.x == 0) { out2[0] = a; out2[1] = b; }
}

static long long seg_of(long long n) { const long long s = (n + AL_PARTS - 1) / AL_PARTS; return s < 1 ? 1 : s; }

}  // namespace mr

using namespace mr;

extern "C" long long mirres_albedo_scratch_bytes(void) { return MIRRES_ALBEDO_SCRATCH_BYTES; }

extern "C" int mirres_albedo_compact(const float* pred, const float* gt_rgba, long long n, double mask_thr, float* pool_pred, float* pool_gt, long long pool_cap,
                                     unsigned long long* state, void* scratch, void* stream) {
    if (n < 0 || pool_cap < 0 || !state || !scratch || (n > 0 && (!pred || !gt_rgba)) || (pool_cap > 0 && (!pool_pred || !pool_gt)) || !(mask_thr == mask_thr)) {
        set_error("mirres_albedo_compact: bad argument (n %lld, pool capacity %lld)", n, pool_cap); return MIRRES_E_ARG;
    }
    if (n == 0) return MIRRES_OK;
    hipStream_t s = (hipStream_t)stream;
    u64* counts = reinterpret_cast<u64*>(scratch);
    const long long seg = seg_of(n);
    k_compact_count<<<AL_PARTS, AL_BLOCK, 0, s>>>(gt_rgba, n, seg, mask_thr, counts, state);
    k_compact_scan<<<1, AL_BLOCK, 0, s>>>(counts, state, (u64)pool_cap);
    k_compact_scatter<<<AL_PARTS, AL_BLOCK, 0, s>>>(pred, gt_rgba, n, seg, mask_thr, counts, pool_pred, pool_gt, (u64)pool_cap);
    MR_LAUNCH_CHECK("albedo_compact");
    return MIRRES_OK;
}

extern "C" int mirres_albedo_median(const float* pool_pred, const float* pool_gt, long long count, double* out3, void* scratch, void* stream) {
    if (count <= 0) { set_error("mirres_albedo_median: the pool is empty (no pixel passed the mask): there is no median"); return MIRRES_E_ARG; }
    if (count >= (1LL << 40) || !pool_pred || !pool_gt || !out3 || !scratch || ((uintptr_t)pool_pred & 15) || ((uintptr_t)pool_gt & 15)) {
        set_error("mirres_albedo_median: bad argument (count %lld; the pools must be 16-byte aligned)", count); return MIRRES_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    AlScratch* sc = reinterpret_cast<AlScratch*>(scratch);
    const u64 n = (u64)count;
    const int grid = (int)std::min<u64>(AL_GRID, ((n + 3) / 4 + AL_BLOCK - 1) / AL_BLOCK);
    k_select_init<<<1, AL_BLOCK, 0, s>>>(sc, (n - 1) / 2);
    for (int shift = 56; shift >= 0; shift -= 8) {
        k_select_hist<<<grid, AL_BLOCK, 0, s>>>(pool_pred, pool_gt, n, shift, sc);
        k_select_pick<<<1, AL_BINS, 0, s>>>(sc, shift);
    }
    if (!(n & 1)) k_select_next<<<grid, AL_BLOCK, 0, s>>>(pool_pred, pool_gt, n, sc);
    k_select_finish<<<1, 64, 0, s>>>(sc, n, out3);
    MR_LAUNCH_CHECK("albedo_median");
    return MIRRES_OK;
}

extern "C" int mirres_albedo_score(const float* pred, const float* gt_rgba, long long n, double mask_thr, const double* h_scale3, double* out_sums2,
                                   uint8_t* out_pred_u8, uint8_t* out_gt_u8, void* scratch, void* stream) {
    if (n <= 0 || !pred || !gt_rgba || !out_sums2 || !scratch || !(mask_thr == mask_thr)) { set_error("mirres_albedo_score: bad argument (n %lld)", n); return MIRRES_E_ARG; }
    hipStream_t s = (hipStream_t)stream;
    double* partial = reinterpret_cast<double*>(scratch);
    const double s0 = h_scale3 ? h_scale3[0] : 1.0, s1 = h_scale3 ? h_scale3[1] : 1.0, s2 = h_scale3 ? h_scale3[2] : 1.0;
    k_score<<<AL_PARTS, AL_BLOCK, 0, s>>>(pred, gt_rgba, n, seg_of(n), mask_thr, s0, s1, s2, partial, out_pred_u8, out_gt_u8);
    k_score_sum<<<1, AL_BLOCK, 0, s>>>(partial, out_sums2);
    MR_LAUNCH_CHECK("albedo_score");
    return MIRRES_OK;
}
