/* gptq_gguf_levels.h -- the one-pass level build of libgptqgguf_hip.so: an additive extension of the C ABI of
   gptq_gguf.h (same library, same conventions: status codes, gq_last_error, device pointers, `stream` a hipStream_t).
   GQ_ABI_VERSION does not change.  The symbol lives in a header of its own so that gptq_gguf.h stays the symbol set
   its version names. */
#ifndef GPTQ_GGUF_LEVELS_H
#define GPTQ_GGUF_LEVELS_H

#include "gptq_gguf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the column walk of gq_gptq_quantize over row BANDS of different K-quant types that share U.

   The level database of the bit-width search holds every Linear at Q2_K .. Q6_K.  The Hessian, its factorisation and the
   C dependent steps of the column walk do not depend on the level; only the grid a row is rounded to does.  So the levels
   of a Linear (and of the Linears that share its U) are working copies of W stacked by rows, each band with its type:

     W        [R, C] fp32, the working copies one under the other; becomes the dequantized matrices
     bands    HOST array, read during the call (it travels in the kernel arguments: no staging copy is put on the stream):
              band k is rows [bands[k-1].row_end, bands[k].row_end) and is quantized to bands[k].q_type
              (GQ_Q2_K .. GQ_Q6_K).  row_end ascending, every row_end % 64 == 0, the last one == R, 1 <= n_bands <=
              GQ_BANDS_MAX.  A type may appear in several bands.
     qweight  [R, C] bytes (for Q3_K / Q6_K bands the byte is an int8, as gq_gptq_quantize leaves it)
     d, dmin  [R, C / 256] fp16 bit patterns
     s, m     the bands' [rows_k, C / G_k] arrays concatenated in band order: band k starts at byte
              sum_{j < k} rows_j * C / G_j  (G = 16 for Q2_K / Q3_K / Q6_K, 32 for Q4_K / Q5_K), R * C / 16 bytes at most
     ws       gq_workspace_bytes(GQ_WS_GPTQ_QUANTIZE, R, C, 0, block_size) bytes

   Contract: every band's rows of qweight, d, s, dmin, m and of W are bit-identical to gq_gptq_quantize called on that
   band's rows alone with that type, static_groups = 0 and the same U (for Q3_K / Q6_K bands dmin / m are what that call
   leaves there).  The panel-wide `continue` of quant_utils.py:250-252 -- the one place the reference looks across rows --
   is evaluated per band.

   One walk: per 256 columns the call issues the column-loop launches, near updates and far updates of a single-type call
   on [R, C] (pair path, look-ahead super-blocks and the far helper included); a workgroup of the column-loop kernel owns
   64 rows, lies in one band and takes group size, signedness, clamp and its s / m base from the band table.  Only the lazy
   scale search at each 256-column boundary is one launch per band, on W as it is at that column.

   No static groups, no act_order, no row slices.  A bad table is GQ_E_BAD_SHAPE (GQ_E_BAD_TYPE for an unknown type),
   a short workspace GQ_E_WORKSPACE, each with a gq_last_error text; every check is made before the first HIP call: a
   refused call has launched nothing and written nothing.  The call only enqueues. */
#define GQ_BANDS_MAX 64

typedef struct {
    int64_t row_end;
    int32_t q_type;
} gq_band_t;

int gq_gptq_quantize_bands(float* W, const float* U, int64_t R, int64_t C, const gq_band_t* bands_host, int n_bands,
                           int block_size, const gq_search_t* p_host, uint8_t* qweight, uint16_t* d, uint8_t* s,
                           uint16_t* dmin, uint8_t* m, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
