// gq_levelpack.hip -- K19: the outputs of one banded column walk (gq_gptq_quantize_bands) as GGUF block bytes, every band
// into a buffer of its own, in ONE launch.  The host path it replaces runs, per band, a row permute of five tensors (q / k)
// and one gq_pack launch.
//
// The band table travels in the kernel arguments (PackTable, 3120 bytes of the 4 KB segment at GQ_BANDS_MAX bands): no
// staging buffer, no copy on the stream.  Entry k carries the prefix sum `unit_end` of work units of bands 0 .. k;
// workgroup u (one unit) finds its band by a binary search over that column -- block-uniform values, i.e. scalar loads
// from the argument segment -- and runs ONE turn of gq_pack's kernel for that band's type:
//   a unit is PB = 32 consecutive OUTPUT blocks of a band, so its nb * type_size output bytes are contiguous and start 16-byte
//   aligned whatever the type (32 * type_size % 16 == 0): the 110- / 210-byte layouts, whose odd blocks are 2-byte aligned,
//   leave through the LDS image as 16-byte stores, the others as coalesced dwords (pack_store, gq_pack_layout.hpp).
//   Output block b is row b / per_row of the band; with a gather its input row is row_src[row], so the input side is per_row
//   contiguous blocks at a time: each block's 256 codes are 16 lanes x 16 bytes whichever row they come from, the s / m / d
//   indices follow the same source block.  The source block of each of the unit's blocks is resolved once into LDS.
// HBM-bound like gq_pack: 1 B/param in (+ scales), type_size / 256 B/param out.
#include "../../../include/gptq_gguf_levelpack.h"
#include "../gq_pack_layout.hpp"

namespace gq {
namespace {

struct PackBand {
    uint8_t* out;
    const int32_t* row_src;
    int64_t blk0;       // first 256-value block of the band in the stacked inputs (row0 * per_row)
    int64_t nblk;       // blocks of the band (rows * per_row)
    int64_t sm_off;     // byte offset of the band's s (and m) array
    uint32_t unit_end;  // work units of bands 0 .. this one
    int32_t q_type;
};
struct PackTable {
    const uint8_t* q;
    const uint16_t* d;
    const uint8_t* s;
    const uint16_t* dmin;
    const uint8_t* m;
    int32_t per_row;  // blocks per row (C / 256)
    int32_t n;
    PackBand b[GQ_BANDS_MAX];
};
static_assert(sizeof(PackTable) <= 4096 - 64, "the band table must fit the kernel-argument segment");

constexpr int TS_MAX = 210, NG_MAX = 16;

template <int QT, int TS, int NG>
__device__ __forceinline__ void band_turn(const PackTable& t, const PackBand& B, int64_t b0, uint8_t* sq, uint8_t* so, uint8_t* ss,
                                          uint8_t* sm, uint16_t* sd, uint16_t* sdm, int64_t* ssrc) {
    constexpr bool MIN = QT == GQ_Q2_K || QT == GQ_Q4_K || QT == GQ_Q5_K;  // the types with dmin / m
    const int tid = threadIdx.x;
    const int nb = (int)((B.nblk - b0) < PB ? (B.nblk - b0) : PB);
    if (tid < nb) {  // where output block b0 + tid comes from
        const int64_t ob = b0 + tid, r = ob / t.per_row, c = ob - r * t.per_row;
        const int64_t sr = B.row_src ? (int64_t)B.row_src[r] : r;
        const int64_t lb = sr * t.per_row + c;  // block within the band
        ssrc[tid] = lb;
        sd[tid] = t.d[B.blk0 + lb];
        sdm[tid] = MIN ? t.dmin[B.blk0 + lb] : (uint16_t)0;
    }
    __syncthreads();
    {  // nb * 256 code bytes = nb * 16 uint4: two loads per thread before the first LDS write
        const int n16 = nb * 16;
        uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
        if (tid < n16) v0 = reinterpret_cast<const uint4*>(t.q + (B.blk0 + ssrc[tid >> 4]) * 256)[tid & 15];
        if (tid + 256 < n16) v1 = reinterpret_cast<const uint4*>(t.q + (B.blk0 + ssrc[(tid + 256) >> 4]) * 256)[tid & 15];
        if (tid < n16) reinterpret_cast<uint4*>(sq)[tid] = v0;
        if (tid + 256 < n16) reinterpret_cast<uint4*>(sq)[tid + 256] = v1;
    }
    for (int i = tid; i < nb * NG; i += 256) {
        const int64_t g = B.sm_off + ssrc[i / NG] * NG + i % NG;
        ss[i] = t.s[g];
        sm[i] = MIN ? t.m[g] : (uint8_t)0;
    }
    __syncthreads();
    pack_store<QT, TS, NG>(sq, so, ss, sm, sd, sdm, nb, B.out + b0 * TS);
}

__global__ __launch_bounds__(256) void pack_bands_kernel(const PackTable t) {
    __shared__ __attribute__((aligned(16))) uint8_t sq[PB * 256];
    __shared__ __attribute__((aligned(16))) uint8_t so[PB * TS_MAX];
    __shared__ __attribute__((aligned(16))) uint8_t ss[PB * NG_MAX];
    __shared__ __attribute__((aligned(16))) uint8_t sm[PB * NG_MAX];
    __shared__ uint16_t sd[PB], sdm[PB];
    __shared__ int64_t ssrc[PB];
    const uint32_t u = blockIdx.x;
    int lo = 0, hi = t.n - 1;  // the first band whose unit_end exceeds u (the grid is b[n - 1].unit_end: it exists)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u < t.b[mid].unit_end) hi = mid;
        else lo = mid + 1;
    }
    const PackBand& B = t.b[lo];
    const int64_t b0 = (int64_t)(u - (lo ? t.b[lo - 1].unit_end : 0u)) * PB;  // the unit's first block within the band
    switch (B.q_type) {
    case GQ_Q2_K: band_turn<GQ_Q2_K, 84, 16>(t, B, b0, sq, so, ss, sm, sd, sdm, ssrc); break;
    case GQ_Q3_K: band_turn<GQ_Q3_K, 110, 16>(t, B, b0, sq, so, ss, sm, sd, sdm, ssrc); break;
    case GQ_Q4_K: band_turn<GQ_Q4_K, 144, 8>(t, B, b0, sq, so, ss, sm, sd, sdm, ssrc); break;
    case GQ_Q5_K: band_turn<GQ_Q5_K, 176, 8>(t, B, b0, sq, so, ss, sm, sd, sdm, ssrc); break;
    default: band_turn<GQ_Q6_K, 210, 16>(t, B, b0, sq, so, ss, sm, sd, sdm, ssrc); break;
    }
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_pack_bands(const uint8_t* qweight, const uint16_t* d, const uint8_t* s, const uint16_t* dmin, const uint8_t* m,
                  int64_t R, int64_t C, const gq_band_t* bands_host, int n_bands, void* const* outs_host,
                  const int32_t* const* row_srcs_host, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!bands_host) GQ_FAIL(GQ_E_NULL, "gq_pack_bands: null band table");
    if (!outs_host) GQ_FAIL(GQ_E_NULL, "gq_pack_bands: null outs");
    if (!qweight || !d || !s) GQ_FAIL(GQ_E_NULL, "gq_pack_bands: null qweight / d / s");
    if (n_bands < 1 || n_bands > GQ_BANDS_MAX) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_bands: %d bands (1..%d)", n_bands, GQ_BANDS_MAX);
    if (R <= 0 || C <= 0 || C % 256 || C / 256 > INT32_MAX)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_bands: R=%ld C=%ld (C %% 256 != 0)", (long)R, (long)C);
    if (!aligned(qweight, 16) || !aligned(d, 2) || !aligned(dmin, 2))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_bands: qweight must be 16-byte, d / dmin 2-byte aligned");
    PackTable t{};  // every check first: a refused call has launched nothing
    t.q = qweight, t.d = d, t.s = s, t.dmin = dmin, t.m = m;
    t.per_row = (int32_t)(C / 256), t.n = n_bands;
    int64_t prev = 0, off = 0, units = 0;
    for (int k = 0; k < n_bands; ++k) {
        const int64_t e = bands_host[k].row_end;
        TypeInfo tk;
        if (!type_info(bands_host[k].q_type, tk))
            GQ_FAIL(GQ_E_BAD_TYPE, "gq_pack_bands: band %d has unknown q_type %d", k, (int)bands_host[k].q_type);
        if (e % 64 || e <= prev || e > R)
            GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_bands: band %d ends at row %ld (ascending multiples of 64 up to R=%ld)", k, (long)e, (long)R);
        if (tk.k_search && (!dmin || !m)) GQ_FAIL(GQ_E_NULL, "gq_pack_bands: band %d of q_type %d needs dmin / m", k, (int)bands_host[k].q_type);
        if (!outs_host[k]) GQ_FAIL(GQ_E_NULL, "gq_pack_bands: band %d: out is NULL", k);
        if (!aligned(outs_host[k], GQ_PACK_BANDS_ALIGN))
            GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_bands: band %d: out not %d-byte aligned", k, GQ_PACK_BANDS_ALIGN);
        const int32_t* rs = row_srcs_host ? row_srcs_host[k] : nullptr;
        if (!aligned(rs, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_bands: band %d: row_src not 4-byte aligned", k);
        PackBand& b = t.b[k];
        b.out = static_cast<uint8_t*>(outs_host[k]), b.row_src = rs;
        b.blk0 = prev * t.per_row, b.nblk = (e - prev) * t.per_row, b.sm_off = off, b.q_type = bands_host[k].q_type;
        units += (b.nblk + PB - 1) / PB;
        if (units > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_bands: R=%ld C=%ld is more than one launch takes", (long)R, (long)C);
        b.unit_end = (uint32_t)units;
        off += (e - prev) * (C / tk.group);
        prev = e;
    }
    if (prev != R) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_bands: the last band ends at row %ld, R=%ld", (long)prev, (long)R);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PT_PACK, st);
    hipLaunchKernelGGL(pack_bands_kernel, dim3((unsigned)units), dim3(256), 0, st, t);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
