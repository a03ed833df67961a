/* libpaths_hip.so — C ABI of the MI355X (gfx950) PATHS hot path.
 *
 * The reference (zzbuzzard/PATHS) is pure Python/PyTorch and has NO FFI of its own; this header is the
 * thin boundary the build defines underneath the reference's Python surface.  Each entry
 * point names the reference code it replaces (file:line relative to the reference repo root).
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is a DEVICE pointer unless stated; no torch types.  Stated exceptions: the grid base
 *     addresses in grid_ptrs of paths_level0_batch* / paths_gather_rows* and the row addresses paths_stage_rows follows may be
 *     PINNED, device-mapped host addresses (hipHostMalloc / torch pin_memory; never pageable or managed memory);
 *   - returns 0 on success, a negative code on error (-1 invalid argument, -2 launch failure,
 *     -3 unsupported configuration); paths_last_error() returns a thread-local message;
 *   - never allocates, frees or synchronises; launches on the caller's stream (hipStream_t passed as
 *     void*); no global mutable state, callable from any host thread;
 *   - paths_stream_t is void* for every consumer.  A translation unit that has the HIP runtime's types may define
 *     PATHS_STREAM_T (as hipStream_t) before it includes this header; the library's own sources do (csrc/common.h), so the
 *     compiler checks every definition against the declaration here.  The ABI is the same either way: one pointer.  This header
 *     is also the only statement of the signatures: the Python binding (paths_amd/_lib.py) reads argument and return types from
 *     it, so a declaration is `<int | int64_t | void* | const char*> paths_name(<parameters>);` with named parameters of type
 *     int, int64_t, float, uint32_t, uint64_t, size_t, a pointer or paths_stream_t;
 *   - all floating-point buffers are fp32, row-major, 16-byte aligned, leading dimensions in elements
 *     and multiples of 4; integer fields follow the reference's dtypes (int64 locs / num_ims /
 *     parent_inds);
 *   - arithmetic: fp32 inputs, outputs and accumulation everywhere.  The *_x6 / *_h3 entry points multiply SPLIT operands on
 *     the 16-bit matrix cores: planes = 2 -> x = hi + lo as two fp16 planes (22 significant bits; 3 x
 *     v_mfma_f32_32x32x16_f16 per product block; operands pre-scaled by powers of two, w_scale / a_scale arguments, and
 *     |activation| * a_scale must stay below 65504: the Python host checks max|x| of every resident grid / input batch
 *     (paths_tissue_mask_absmax) and runs out-of-range data on planes = 3); planes = 3 -> x = hi + mid + lo EXACTLY as three
 *     bf16 planes (6 x v_mfma_f32_32x32x16_bf16, no range limits).  The entry points without suffix use the f32-input
 *     matrix cores (v_mfma_f32_32x32x2_f32 / 16x16x4_f32: a k-ordered fp32 FMA chain).  Measured error of all three vs
 *     fp64 is that of an fp32 FMA chain.
 *
 * UNDEFINED MEMORY.  What a buffer may hold on entry where its contents are not an operand: rows of padding (row index within the
 * slide >= num_ims[b]; token rows >= num_ims[b] + 1), pad columns between a row's width and its leading dimension, workspaces and
 * operand images, zones a kernel may read behind a buffer.  Four phrases, each with the meaning tests/test_gpu_undefined_memory.py
 * asserts (the defined part of every output is BIT-identical whatever such memory held; no float atomics anywhere):
 *   never read                     the bytes are not loaded, or every byte that is loaded was written by this call first;
 *   read, any bit pattern          loaded, and no defined output depends on them: NaN, Inf and 0xff bytes included;
 *   read, must be finite           loaded and multiplied by exact zeros: any finite value leaves every defined output as it is,
 *                                  a NaN or an infinity does not;
 *   must be zero on entry          (written by ...): a precondition.
 * OUTPUT rows of padding are what each entry point says below; where it says nothing they are not defined (written from whatever the
 * padded input rows held, or not written at all when tiles of padding are skipped).  Pad columns [width, ld) of every strided
 * operand: never read, never written.  Rows past the M / B * T rows of an operand: never read unless stated.
 *
 * attention, forward
 *   paths_attention_x6 / _x6_dropout   q, k, v rows of padding: read, any bit pattern (they enter the operand images as zeros - the
 *                                      keys because they are masked, the queries because their scores share the wave-wide votes of
 *                                      the deferred rescale with valid queries); workspace on entry (images_ready = 0): never read;
 *                                      images_ready != 0: the images of paths_token_layer_h3 / _ws / paths_importance_qkv_x6, whose
 *                                      writers zero the same rows in every 64-token tile that holds a valid token (other tiles:
 *                                      never read); o / lse rows of padded queries: not defined
 *   paths_attention_f32                q, k, v rows of padding: read, any bit pattern
 *   paths_attention_any / _any_train / _h3_any / paths_attention_token0_any / paths_attention_fp8 / _fp8_qkv / paths_attention_token0_fwd
 *                                      q | k | v rows of padding: read, any bit pattern; workspace on entry: never read
 *   paths_attention_wide_fwd           qkv rows of padding: read, must be finite (O = P V multiplies v by the zero probabilities of
 *                                      masked keys); the 128 rows behind qkv: read, any bit pattern; workspace on entry: never read
 * attention, backward (dqkv: must be zero on entry, written by the caller, for every entry point)
 *   paths_attention_bwd_f32 / _f32_dropout     k, v, lse rows of padding: read, any bit pattern; q, o, d_o rows of padding: read, must
 *                                              be finite (D = sum dO o of a padded query and its q and dO rows meet zero
 *                                              probabilities inside the matrix products); ws_dsum on entry: never read
 *   paths_attention_bwd_x6_planes / _x6_dropout  q, k, v, lse rows of padding: read, any bit pattern; o, d_o rows of padding: read,
 *                                              must be finite; ws_dsum, images on entry: never read
 *   paths_attention_bwd_any / paths_attention_token0_bwd   every input's rows of padding: read, any bit pattern; ws_dsum / ws: never read
 *   paths_attention_wide_bwd           qkv and d_o rows of padding: read, must be finite; o, lse rows of padding: never read; the
 *                                      128 rows behind qkv: read, any bit pattern; workspace on entry: never read
 *   The training step computes rows of padding instead of skipping them (paths_amd/utils.py:recurse_train), so every saved row is finite.
 * token-layer chain
 *   paths_token_layer_f32 / _h3 / _ws / _ws_rows   x_in and attn rows of padded tokens: read, any bit pattern (skip_padding 0: each is
 *                                      computed into the same row of the outputs; 1: 64-token tiles of padding are skipped);
 *                                      qkv_images, q, k, v, qkv_rows, x_out on entry: never read
 *   paths_attention_h3_img / paths_attention_h3_any_img   o_img / o on entry: never read; workspace: the producer's images
 *   paths_token0_tail                  x_in, q, k, v rows of padded tokens: read, any bit pattern; ws_partials on entry: never read
 *   paths_token0_tail_ws               x1 rows of padded tokens: read, any bit pattern; partials on entry: never read; counters: must
 *                                      be zero on entry (written by the caller once; every launch leaves them zero)
 * gate and importance GEMMs
 *   paths_lstm_cell_x6 / _h16 with num_ims    rows of x (or the rows x_rows addresses), h0, c0 of padded patches: read, any bit
 *                                      pattern; ws_o and every output on entry: never read; every row of hp counts
 *   paths_importance_proj_x6 / _h16, paths_importance_qkv_x6 / _h16   rows of y (or the rows y_rows addresses) and y_add of padded
 *                                      patches: read, any bit pattern; splitk_ws, qkv_images on entry: never read; importance of a
 *                                      padded row is +0.0 (skip_padding 0) or not written (1)
 *   paths_gemm_add_nt_x6 / _h16 with num_ims  rows of a (a_rows) and a_add of padded patches: read, any bit pattern
 *   paths_gemm_rows_nt_x6              every address of a_rows is read: none is padding
 * reductions over rows (they sum over M without a mask, by design)
 *   paths_gemm_tn_f32 / _tn_x6, paths_colsum_f32, paths_reduce_slabs_f32, paths_layernorm_bwd_sums / _any
 *                                      EVERY row of a, b0 | b1, dy, xhat, rstd and every slab counts: the caller hands over defined
 *                                      (for padding: zero) rows; workspace / slabs / dx on entry: never read; out with
 *                                      accumulate = 0: never read
 * row backward kernels
 *   paths_lstm_bwd_a / _b              dh1, dh1b, o, tc, dc1_h, dc1_ext, frm, c0 rows of padded patches: read, any bit pattern
 *   paths_importance_bwd / _any        dtok rows of padded patches and of the special token: read, any bit pattern; pproj, hid: saved
 *                                      activations, finite in every row
 *   paths_importance_rows_bwd / _any   dz_rows and x rows of padded patches: read, any bit pattern
 * packers and pack kernels
 *   paths_x6_pack_weights / _t, paths_tlayer_pack_ws, paths_tlayer_pack_h3, paths_token0_pack_ws / _d, paths_fp8_pack_weight
 *                                      write EVERY byte of an image of the queried size (padding rows and columns as zeros): out on
 *                                      entry: never read, and a consumer never sees what the buffer held
 *   paths_pack_flags / _index / _rows  flags, index, count, partials, rows on entry: never read (flags is written in full by
 *                                      paths_pack_flags before paths_pack_index counts it)
 * heat-map rasters
 *   paths_raster_index                 locs rows of padding: never read; index: must be -1 on entry, status: must be zero on entry
 *                                      (both written by the caller)
 *   paths_raster_maps                  value rows of padding: never read (only rows an index grid names are); out on entry: never
 *                                      read, every element of the padded allocation is written
 *   paths_render_range                 raster cells no drawn index grid names: never read; partial, range, status on entry: never
 *                                      read (status is written, not accumulated)
 *   paths_render_rgb                   raster cells no drawn index grid names, thumbnail bytes outside a slide's extent: never read;
 *                                      out on entry: never read, every byte of the padded allocation is written
 * annotation polygons
 *   paths_polygon_cover                words between the packed arrays (behind verts[V], poly_off[P], slide_poly[B]): never read; out on
 *                                      entry: never read, every element of the padded allocation is written
 *   paths_polygon_outline              words between the packed arrays and cum behind cum[V]: never read; image bytes: never read;
 *                                      bytes of pixels no edge paints, row padding included: never written
 * row cache of on-demand slides
 *   paths_cache_probe                  cells beyond n[b]: never read; src, miss_count, miss_cells, status on entry: never read
 *   paths_cache_fill / _h16            src beyond n[b], store rows at and beyond count[b], out on entry: never read; every row of out
 *                                      is written
 * pixels to encoder input
 *   paths_grey_histogram               image bytes behind a row's cols * 3 (row padding): never read; partials, counts, status on entry:
 *                                      never read
 *   paths_tile_tissue                  tile bytes outside the P x 3P window (row padding, neighbouring tiles): never read; counts, flags
 *                                      on entry: never read
 *   paths_tile_compact                 order, m, slot, status on entry: never read; order at and beyond m: not written
 *   paths_tiles_to_input               tile bytes outside the P x 3P window: never read; order outside [first, first + count), so every
 *                                      entry beyond m: never read; out on entry: never read, every element is written
 *   paths_tiles_resize_to_input        tile bytes outside the P x 3P window: never read; order outside [first, first + count): never
 *                                      read; bounds / coef: whatever they hold, only bytes of the window and LDS the workgroup wrote
 *                                      are read; out on entry: never read, every element is written
 *   paths_scatter_rows                 enc rows at and beyond m: never read; out on entry: never read, every row is written
 */
#ifndef PATHS_HIP_H
#define PATHS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PATHS_STREAM_T
#define PATHS_STREAM_T void*
#endif
typedef PATHS_STREAM_T paths_stream_t; /* hipStream_t */

const char* paths_last_error(void);
const char* paths_build_info(void);
/* 3: paths_importance_qkv_x6 / _h16 take no top-K arguments (keep .. status) any more.  2 since round 5.  Differences a consumer built against ABI 1 must know: (a) dropout masks (paths_dropout_mask and every *_dropout /
 * drop_key entry) are one 16-bit hash half per element - thr16 = round(p * 65536) clamped to [1, 65535] for p > 0, kept elements scaled by
 * 1 / (1 - thr16 / 65536), attention mask rows T rounded up to even elements apart - so the same (key, p) yields other masks than ABI 1;
 * p >= 1 is rejected by every entry point (p in (1 - 2^-16, 1) is applied as 65535 / 65536); (b) events of paths_event_create order
 * streams of ONE device (created with hipEventDisableSystemFence): never wait for them on the host. */
int paths_abi_version(void);

/* Stream plumbing of the launch tape (paths_amd/utils.py:TapedRecursion replays a recorded recursion as a flat list of C calls;
 * no reference equivalent).  paths_event_create / paths_event_destroy: a timing-less event handle (host object) for paths_stream_wait, which makes `dst`
 * wait for everything enqueued on `src` so far; paths_memset_zero: hipMemsetAsync(0).  None of them synchronises the host. */
void* paths_event_create(void);
/* a HIP stream restricted to the compute units set in cu_mask (words x 32 bits): measurement aid (CU-partitioned streams) */
void* paths_stream_create_masked(const uint32_t* cu_mask, int words);
int paths_event_destroy(void* event);
int paths_stream_wait(paths_stream_t dst, paths_stream_t src, void* event);
/* Stop events: paths_set_stop_event(ev) makes the next stop-capable launch of this host thread (the importance / projection finish
 * kernel of paths_importance_proj_x6, the kernel of paths_topk / paths_topk_rows and of their _tiled forms) carry ev as its completion event - no event-record
 * packet of its own in the launching queue; paths_flush_stop_event(src) records it on src the ordinary way if no launch took it;
 * paths_stream_wait_event(dst, ev): dst waits for ev.  paths_stop_event_pending(): 1 while the armed event has not been taken;
 * paths_clear_stop_event(): disarm without recording (error paths); paths_record_event(ev, s): plain hipEventRecord - the caller
 * re-records ev behind launches that followed the stop-capable kernel, so the join covers them too (paths_amd/_lib.py:fork_behind). */
int paths_set_stop_event(void* event);
int paths_flush_stop_event(paths_stream_t src);
int paths_stop_event_pending(void);
int paths_clear_stop_event(void);
int paths_record_event(void* event, paths_stream_t stream);
int paths_stream_wait_event(paths_stream_t dst, void* event);
int paths_memset_zero(void* p, size_t bytes, paths_stream_t stream);

/* LSTMCell.forward over depth + residual (reference model/interface.py:31-58, model/paths.py:78-91).
 *   x [M,D] (ldx), h0/c0 = previous state views (both NULL at depth 0), M = B * rows_per_slide.
 *   w_gates [3Hc+D, 2D] PACKED: rows [0,3Hc) in groups of 96 = forget|remember|map rows of one block of
 *   32 memory units, rows [3Hc, 3Hc+D) = out_select_gate; b_gates packed alike; w_mem [D,Hc], b_mem [D].
 *   state_out [M, D+Hc] <- (h1 | c1)  (= "ctx_patch"), y [M,D] <- x + h1, ws_o [M,D] scratch.
 *   num_ims != NULL: tiles that contain only padding rows (row index within slide >= num_ims[b]) are skipped.
 *   phases: bit0 memory-cell GEMM, bit1 output-gate GEMM, bit2 mem_to_out GEMM; pass 7 (all, in this order).
 *   save_frm [M,3Hc] / save_tc [M,D] (both optional): gate activations f|r|m (packed order) and tanh(Wc c1 + bc),
 *   kept for the backward pass; ws_o then holds the output gate o.
 *   hp [rows, 3Hc+D] + hp_row [M] (optional, instead of h0): siblings share their parent's h, so h_parent Wh^T is computed
 *   ONCE per kept parent (paths_gather_kept_rows + paths_gemm_nt_f32 on w_gates[:, D:2D]) and added in the epilogue
 *   through hp_row (-1 = no parent: zero state); the gate GEMM then only runs over the x panel (K = D). */
int paths_lstm_cell(const float* x, int64_t ldx, const float* h0, int64_t ldh0, const float* c0, int64_t ldc0,
                    const float* w_gates, const float* b_gates, const float* w_mem, const float* b_mem,
                    float* state_out, int64_t ldso, float* y, int64_t ldy, float* ws_o, float* save_frm, float* save_tc,
                    const float* hp, const int* hp_row,
                    int M, int D, int Hc, const int64_t* num_ims, int rows_per_slide, int phases, paths_stream_t stream);

/* importance MLP + sigmoid + padding mask, importance scaling, proj_in, positional encoding, special token
 * (reference model/paths.py:95-98,119-124; utils.py:16-23,47-67,106-115; model/aggregator.py:37-65).
 *   w_ip [256, D] = importance_mlp.0.weight (W1) and proj_in.weight (Wp) interleaved in blocks of 64 rows:
 *   [W1[0:64] ; Wp[0:64] ; W1[64:128] ; Wp[64:128]]; b1 / w2 / bp in their natural order; tokens [B, N+1, d]: row 0 = special token.
 *   pe_mode 2 = "2d" (div_term has d/4 entries, locs [M,2] int64 pixel coords), 1 = "1d" (d/2 entries).
 *   pe_table (optional) = paths_pe_table output with pe_rows rows: sin/cos values are then read from it (bit-identical to
 *   evaluating them).  The caller guarantees 0 <= locs / patch_size < pe_rows (paths_amd passes the level's grid size);
 *   positions are clamped into the table for memory safety only. */
int paths_pe_table(const float* div_term, int pe_mode, int d, int rows, float* out, paths_stream_t stream);
int paths_importance_proj(const float* y, int64_t ldy, const float* w_ip, const float* b1, const float* w2, const float* b2 /* device scalar */,
                          const float* bp, const float* special, const float* div_term, const float* pe_table, int pe_rows,
                          const int64_t* locs,
                          const int64_t* num_ims, int rows_per_slide, int patch_size, int pe_mode, int imp_mul,
                          float* importance, float* tokens, float* save_hid, float* save_pproj, int M, int D, int Hi, int d,
                          int skip_padding, paths_stream_t stream);

/* ---- split-operand variants of the three GEMM entry points above: same arithmetic contract (fp32 in, fp32 out, fp32
 * accumulation, error of the order of an fp32 FMA chain's), computed on the 16-bit matrix cores (csrc/gemm_x6.hip).
 *   planes = 3 ("x6"): every fp32 operand is the exact sum of three bf16 (hi+mid+lo); six of the nine partial products are
 *                      kept (dropped: <= 2^-25 |a w|); 6 bf16 MFMAs per product block.  No range restrictions; scales must be 1.
 *   planes = 2 ("h3"): operands are split into two fp16 (hi+lo, 22 significant bits); hi*hi + hi*lo + lo*hi are kept (dropped:
 *                      <= 2^-22 |a w|); 3 fp16 MFMAs per product block.  fp16's exponent range is narrow, so operands are
 *                      pre-scaled by powers of two: weights by w_scale when packed (max|w| w_scale < 65504), activations by
 *                      a_scale inside the kernel (|activation| a_scale < 65504; below 0.125 / a_scale the lo plane is
 *                      subnormal: absolute error 2^-25 / a_scale per element).  Accumulators are un-scaled in the epilogues.
 *   planes = 4        (paths_gemm_nt_x6 / paths_x6_pack_weights only): TWO bf16 planes (hi + mid of the exact split: 16
 *                      significant bits per operand, fp32's exponent range: no scales, nothing overflows); hi*hi + hi*mid + mid*hi,
 *                      3 bf16 MFMAs per block, relative error of a product ~2e-5.  The gradient GEMMs of the training step
 *                      (round 3; paths_gemm_tn_x6 has the same form as its planes = 2).
 * Activations stay fp32 in HBM; WEIGHTS are passed as the image produced once by paths_x6_pack_weights:
 *   [Npad/32][K/16][plane][k-half][32 rows][8 x 16 bit]   (paths_x6_packed_bytes(Npad, K, planes) = 2 planes Npad K bytes).
 * They replace the same reference code as their f32 twins (model/interface.py:31-58, model/paths.py:78-98,119-124). */
int64_t paths_x6_packed_bytes(int Npad, int K, int planes);
int paths_x6_pack_weights(const float* w, int64_t ldw, void* out, int N, int Npad, int K, int planes, float w_scale,
                          paths_stream_t stream);
/* The image of W^T made from W: w is [Kvalid, N] fp32 (row stride ldw); the packed weight is [N, K] (rows n >= N and columns k >= Kvalid zero);
 * planes 3 or 4 (bf16 planes, scale 1).  One launch instead of paths_transpose_f32 + paths_x6_pack_weights (the backward's dX products). */
int paths_x6_pack_weights_t(const float* w, int64_t ldw, void* out, int N, int Npad, int K, int Kvalid, int planes, paths_stream_t stream);
/* w_gates_x6 = pack of the PACKED gate matrix [3Hc+D, 2D] of paths_lstm_cell (scale wg_scale); w_mem_x6 = pack of [D, Hc]
 * (scale wm_scale); D % 256 == 0, Hc % 64 == 0 and Hc >= 128 (the mem_to_out product runs over K = Hc and the split-operand
 * GEMM needs K >= 128; paths_lstm_cell takes Hc = 64).  These shape limits and the operand combinations named here are refused
 * before the first launch; alignment and size limits of single operands (ldso % 4, 16-byte alignment of state_out + D, the
 * 4 GiB extent of an operand) are checked by the launch that reads them, so such a refusal may follow earlier phases' writes.
 * y may be NULL (Y = X + h1 not materialised).  x_rows (optional, planes = 2, needs hp / no
 * h0, y = NULL): [M] addresses of the feature rows - x is then read in place (paths_gather_rows row_ptrs), x / ldx unused.
 * ws_o: scratch of ceil(M / 256) * 256 x D floats (with y = NULL and no training saves the output gate crosses from phase 2 to
 * phase 4 as raw pre-activations in whole 32x32 accumulator tiles; otherwise as the [M, D] gate values).
 * Depth 0 (h0, c0, hp and save_frm all NULL, planes = 2): phase 1 computes the remember | map columns only - c0 = 0 never meets the
 * forget gate; same image, same arguments, c1 bit-identical to the three-gate product's with a zero c0. */
int paths_lstm_cell_x6(const float* x, int64_t ldx, const int64_t* x_rows, const float* h0, int64_t ldh0, const float* c0, int64_t ldc0,
                       const void* w_gates_x6, const float* b_gates, const void* w_mem_x6, const float* b_mem,
                       float* state_out, int64_t ldso, float* y, int64_t ldy, float* ws_o, float* save_frm, float* save_tc,
                       const float* hp, const int* hp_row,
                       int M, int D, int Hc, const int64_t* num_ims, int rows_per_slide, int phases,
                       int planes, float wg_scale, float wm_scale, float a_scale, paths_stream_t stream);
/* fp16 slide grids: paths_lstm_cell_x6 with x_rows addressing FP16 feature rows (x = NULL, planes = 2, a_scale a power of two in
 * [1, 2^15]).  The c / o gate GEMMs take a ONE-plane A operand (x a_scale is its own fp16 hi plane, the lo plane is zero): 2 MFMAs per
 * block instead of 3; bit-identical to paths_lstm_cell_x6 on fp32 rows holding the same values. */
int paths_lstm_cell_x6_h16(const float* x, int64_t ldx, const int64_t* x_rows, const float* h0, int64_t ldh0, const float* c0, int64_t ldc0,
                           const void* w_gates_x6, const float* b_gates, const void* w_mem_x6, const float* b_mem,
                           float* state_out, int64_t ldso, float* y, int64_t ldy, float* ws_o, float* save_frm, float* save_tc,
                           const float* hp, const int* hp_row,
                           int M, int D, int Hc, const int64_t* num_ims, int rows_per_slide, int phases,
                           int planes, float wg_scale, float wm_scale, float a_scale, paths_stream_t stream);
/* w_ip_x6 = pack of [256, D] (rows interleaved as for paths_importance_proj); y_add (optional): GEMM input = y + y_add summed
 * in fp32 while staging, so that the caller can pass (x, h1) and skip materialising Y = X + h1; y_rows (optional, planes = 2):
 * row addresses of y instead of (y, ldy) */
int paths_importance_proj_x6(const float* y, int64_t ldy, const int64_t* y_rows, const float* y_add, int64_t ldya, const void* w_ip_x6, const float* b1, const float* w2, const float* b2 /* device scalar */,
                             const float* bp, const float* special, const float* div_term, const float* pe_table, int pe_rows,
                             const int64_t* locs,
                             const int64_t* num_ims, int rows_per_slide, int patch_size, int pe_mode, int imp_mul,
                             float* importance, float* tokens, float* save_hid, float* save_pproj, int M, int D, int Hi, int d,
                             int skip_padding, int planes, float w_scale, float a_scale, float* splitk_ws, paths_stream_t stream);
/* fp16 slide grids: paths_importance_proj_x6 with y_rows addressing FP16 rows (y = NULL; y_add and splitk_ws required, planes = 2):
 * the rows are widened, summed with y_add in fp32 and split as in the fp32 form (split-K form only). */
int paths_importance_proj_x6_h16(const float* y, int64_t ldy, const int64_t* y_rows, const float* y_add, int64_t ldya, const void* w_ip_x6, const float* b1, const float* w2, const float* b2 /* device scalar */,
                                 const float* bp, const float* special, const float* div_term, const float* pe_table, int pe_rows,
                                 const int64_t* locs,
                                 const int64_t* num_ims, int rows_per_slide, int patch_size, int pe_mode, int imp_mul,
                                 float* importance, float* tokens, float* save_hid, float* save_pproj, int M, int D, int Hi, int d,
                                 int skip_padding, int planes, float w_scale, float a_scale, float* splitk_ws, paths_stream_t stream);
/* splitk_ws (optional, paths_importance_proj_x6_workspace(M) bytes; used with planes = 2, y_add given, no training saves): the
 * [M/128 x 1]-block GEMM covers half the chip, so its k loop runs as two halves on twice the blocks (raw accumulators to the
 * workspace) and a second launch sums them and applies the epilogue on 64-row blocks.  null = one launch. */
int64_t paths_importance_proj_x6_workspace(int M);
/* Round 5: paths_importance_proj_x6 (split-K form) AND the first decoder layer's in_proj (paths_token_layer_ws with do_qkv only) as one
 * GEMM + one fused finish, for trans_dim 128 / 4 heads / importance hidden 128, two fp16 planes, N % 64 == 0 (reference
 * model/paths.py:95-98,119-124; model/aggregator.py:37-65 and the self_attn in_proj of decoder layer 0, model/aggregator.py:70-72).
 * TOKEN ORDER of this form: patch i of slide b is token i and the special token sits at index num_ims[b], right behind the valid
 * patches (the reference prepends it; masked self-attention is invariant under that permutation and only the special token's output
 * row is read) - a 64-row block of the GEMM result is then one 64-token tile of the attention's operand images.  Consumers:
 * paths_attention_h3_img, paths_token_layer_ws (position-agnostic) and paths_token0_tail_ws with special_last = 1.
 * phases: bit 1 = the split-K GEMM of (y | y_rows) + y_add into splitk_ws (paths_importance_proj_x6_workspace(B * N) bytes); bit 2 =
 * importance-only finish (alpha -> importance [B, N]); bit 4 = tokens [B, N + 1, 128] + importance (or, alpha_from_importance != 0,
 * importance READ back) + q | k | v operand images of paths_attention_h3_img (qkv_images: paths_attention_x6_workspace(B, N + 1, 4, 32,
 * 2) bytes; w_qkv: paths_tlayer_pack_ws part 1 image with scale s_wqkv, qscale = log2(e) / sqrt(32)).  Bits 2 and 4 are stop-event
 * capable launches and may be issued by separate calls on different streams behind bit 1.  pe_table (paths_pe_table) is required;
 * positions must be < pe_rows (they are clamped for memory safety). */
int paths_importance_qkv_x6(const float* y, int64_t ldy, const int64_t* y_rows, const float* y_add, int64_t ldya, const void* w_ip_x6,
                            const float* b1, const float* w2, const float* b2 /* device scalar */, const float* bp, const float* special,
                            const float* pe_table, int pe_rows, const int64_t* locs, const int64_t* num_ims, int B, int N,
                            int patch_size, int pe_mode, int imp_mul, float* importance, float* tokens, int D, int skip_padding,
                            float w_scale, float a_scale, float* splitk_ws, const void* w_qkv, const float* bqkv, float s_wqkv,
                            float qscale, void* qkv_images, int phases, int alpha_from_importance, paths_stream_t stream);
/* fp16 slide grids: paths_importance_qkv_x6 whose GEMM phase (bit 1) reads y_rows as FP16 rows (y = NULL). */
int paths_importance_qkv_x6_h16(const float* y, int64_t ldy, const int64_t* y_rows, const float* y_add, int64_t ldya, const void* w_ip_x6,
                                const float* b1, const float* w2, const float* b2 /* device scalar */, const float* bp, const float* special,
                                const float* pe_table, int pe_rows, const int64_t* locs, const int64_t* num_ims, int B, int N,
                                int patch_size, int pe_mode, int imp_mul, float* importance, float* tokens, int D, int skip_padding,
                                float w_scale, float a_scale, float* splitk_ws, const void* w_qkv, const float* bqkv, float s_wqkv,
                                float qscale, void* qkv_images, int phases, int alpha_from_importance, paths_stream_t stream);
/* out (+)= maskop(act(a W[:, k0:k0+K]^T + b)) + residual, W = pack of an [Npad, Kpacked] weight; Npad % 128 == 0
 * (256-column tiles when Npad % 256 == 0, else 128-column tiles) */
int paths_gemm_nt_x6(const float* a, int64_t lda, const void* w_x6, int Kpacked, int k0, const float* b, float* out, int64_t ldo,
                     int M, int N, int Npad, int K, int act, const float* residual, int64_t ldr, const float* mask,
                     int64_t ldm, int accumulate, int planes, float w_scale, float a_scale, paths_stream_t stream);
/* out = act((A + A_add) W^T + b), planes = 2: the GEMM input is summed in fp32 while staged (Y = X + h1, reference model/paths.py:89-91,
 * never materialised); A as a matrix or as row addresses (exactly one of a / a_rows); num_ims (optional) skips whole tiles of padding.
 * Npad a multiple of 256 (128 x 256 tiles) or of 192 (128 x 192 tiles: a 320-column product pads to 384 instead of 512). */
int paths_gemm_add_nt_x6(const float* a, int64_t lda, const int64_t* a_rows, const float* a_add, int64_t ld_add, const void* w_x6, int Kpacked,
                         const float* b, float* out, int64_t ldo, int M, int N, int Npad, int K, int act, const int64_t* num_ims,
                         int rows_per_slide, float w_scale, float a_scale, paths_stream_t stream);
/* fp16 slide grids: paths_gemm_add_nt_x6 with a_rows addressing FP16 rows (a = NULL). */
int paths_gemm_add_nt_x6_h16(const float* a, int64_t lda, const int64_t* a_rows, const float* a_add, int64_t ld_add, const void* w_x6, int Kpacked,
                             const float* b, float* out, int64_t ldo, int M, int N, int Npad, int K, int act, const int64_t* num_ims,
                             int rows_per_slide, float w_scale, float a_scale, paths_stream_t stream);
/* The same product without bias / activation, A given as row ADDRESSES (planes = 2 only): row m = the K floats at a_rows[m]. */
int paths_gemm_rows_nt_x6(const int64_t* a_rows, const void* w_x6, int Kpacked, int k0, float* out, int64_t ldo,
                          int M, int Npad, int K, int planes, float w_scale, float a_scale, paths_stream_t stream);

/* ---- backward-pass building blocks (reference: autograd of train.py:65 loss.backward()) --------------------------
 * paths_gemm_nt_f32: out (+)= maskop(act(a W^T + b)) + residual; with W = a transposed weight copy this is dX = dY W.
 * paths_gemm_tn_f32: out[N1,N2] (+)= a[M,N1]^T [b0|b1][M,N2]  (weight gradients; split-M slabs summed in a fixed order).
 * paths_colsum_f32 : out[N] (+)= sum over rows (bias gradients).  paths_transpose_f32: out = in^T. */
int paths_gemm_nt_f32(const float* a, int64_t lda, const float* w, int64_t ldw, const float* b, float* out, int64_t ldo,
                      int M, int N, int Npad, int K, int act, const float* residual, int64_t ldr, const float* mask,
                      int64_t ldm, int accumulate, paths_stream_t stream);
int64_t paths_gemm_tn_workspace(int N1, int N2, int splits);
int paths_gemm_tn_f32(const float* a, int64_t lda, const float* b0, int64_t ldb0, int nb0, const float* b1, int64_t ldb1,
                      float* out, int64_t ldo, int M, int N1, int N2, int splits, int accumulate, float* workspace,
                      paths_stream_t stream);
/* The same product on the bf16 matrix cores, operands split in registers: planes = 3: three exact bf16 planes (6 MFMAs per block, as
 * accurate as the f32 MFMA); planes = 2: hi | mid only (3 MFMAs, 16 significant bits per operand at fp32's exponent range, relative
 * error of a product ~2e-5: the training step's default since round 3).  `splits` is an upper bound (>= 32 rows per split are kept);
 * operands must be smaller than 4 GiB each (32-bit buffer offsets). */
int paths_gemm_tn_x6(const float* a, int64_t lda, const float* b0, int64_t ldb0, int nb0, const float* b1, int64_t ldb1,
                     float* out, int64_t ldo, int M, int N1, int N2, int splits, int accumulate, float* workspace, int planes,
                     paths_stream_t stream);
int paths_colsum_f32(const float* a, int64_t lda, int M, int N, float* out, int splits, int accumulate, float* workspace,
                     paths_stream_t stream);
int paths_transpose_f32(const float* in, int64_t ldi, int R, int C, float* out, int64_t ldo, paths_stream_t stream);

/* Multi-tensor AdamW, one launch per step (replaces torch.optim.AdamW's ~12 foreach launches, reference train.py:49-50 /
 * train.py:66 `opt.step()`; same operation order and fp32 rounding as torch/optim/adam.py:_multi_tensor_adam, so a training
 * trajectory is torch's own bit for bit).  All arrays live in DEVICE memory: table [n][4] addresses (param, grad, exp_avg,
 * exp_avg_sq; fp32 contiguous tensors), numel [n], blocks [nblocks][2] = (tensor index, first element) with
 * paths_adamw_chunk() elements per block, step_size [n] = -lr / (1 - beta1^t), bc2_sqrt [n] = sqrt(1 - beta2^t).
 * wd_scale = 1 - lr * weight_decay (has_wd = 0: no decay), lerp_w = 1 - beta1 (< 0.5), value = 1 - beta2;
 * flavor: bit 0 / 1 / 2 = lerp / addcmul / addcdiv evaluated as ONE fused multiply-add (7 = what the installed torch does). */
int paths_adamw_chunk(void);
int paths_adamw_multi(const int64_t* table, const int64_t* numel, const int32_t* blocks, int nblocks, const float* step_size,
                      const float* bc2_sqrt, float wd_scale, int has_wd, float lerp_w, float beta2, float value, float eps, int flavor,
                      paths_stream_t stream);

/* LSTMCell backward, element-wise parts (reference model/interface.py:52-56 differentiated):
 *   a: dpre_o = dh1 tc o(1-o) -> dG[:, 3Hc:], dpre_h = dh1 o (1-tc^2);  b: packed df|dr|dm -> dG[:, :3Hc], dc0 = dc1 f. */
int paths_lstm_bwd_a(const float* dh1, int64_t ldd, const float* dh1b, int64_t lddb, const float* o, const float* tc,
                     const int64_t* num_ims, int rows_per_slide, int64_t M, int D, float* dpre_o, int64_t ldo,
                     float* dpre_h, paths_stream_t stream);
int paths_lstm_bwd_b(const float* dc1_h, const float* dc1_ext, int64_t lde, const float* frm, const float* c0, int64_t ldc0,
                     const int64_t* num_ims, int rows_per_slide, int64_t M, int Hc, float* dg, int64_t ldg, float* dc0,
                     int64_t lddc0, paths_stream_t stream);
/* importance MLP / scaling backward per patch row (reference model/paths.py:95-98 differentiated). */
int paths_importance_bwd(const float* dtok, const float* pproj, const float* hid, const float* alpha, const float* w2,
                         const int64_t* num_ims, int rows_per_slide, int64_t M, int imp_mul, float* du, float* da, float* dah,
                         paths_stream_t stream);
/* LayerNorm (width 128) forward with saved xhat / rstd, and backward (dx, dy*xhat for the gamma gradient). */
int paths_layernorm_fwd_stats(const float* x, const float* add, const float* gamma, const float* beta, float* y, float* xhat,
                              float* rstd, int64_t rows, int d, float eps, paths_stream_t stream);
int paths_layernorm_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx, float* dyxhat,
                        int64_t rows, int d, paths_stream_t stream);
/* paths_layernorm_bwd without the dy*xhat tensor: every workgroup of rows_per_block rows also writes one 384-float slab
 * sum(dy * xhat) | sum(dy) | sum(dx) of its rows; paths_reduce_slabs_f32 over the ceil(rows / rows_per_block) slabs gives
 * dgamma | dbeta | column sums of dx (the gradient of a bias added in front of the LayerNorm). */
int paths_layernorm_bwd_sums(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx, float* slabs,
                             int64_t rows, int d, int rows_per_block, paths_stream_t stream);
int paths_reduce_slabs_f32(const float* slabs, int splits, int n, float* out, int accumulate, paths_stream_t stream);
/* Deferred slab reductions (csrc/reduce_multi.hip): between paths_defer_reductions(1) and paths_flush_reductions() the final
 * "out (+)= sum of slabs" pass of paths_gemm_tn_f32 / paths_gemm_tn_x6 / paths_colsum_f32 / paths_reduce_slabs_f32 is registered instead
 * of launched; the flush runs all registered reductions in one launch per 32 entries, each in the summation order of the launch it
 * replaces (bit-identical outputs).  The caller keeps the slab workspaces alive until the flush and flushes before anything reads an
 * output; an entry whose output overlaps a pending output or pending slabs flushes first.  Per host thread.  paths_defer_reductions
 * returns the previous setting and does not flush. */
int paths_defer_reductions(int on);
int paths_flush_reductions(int* n_entries, paths_stream_t stream);

/* Self-attention backward, flash style (recompute from q, k, lse; reference: autograd through the attention of
 * model/aggregator.py:70-72).  q is the stored pre-scaled query; gradients land token-major in dqkv [B,T,384] =
 * [dq_scaled | dk | dv] (zero-initialised by the caller); ws_dsum: B*H*T floats. */
int paths_attention_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* d_o, const float* lse,
                            const int64_t* num_ims, float* dqkv, float* ws_dsum, int B, int T, int H, int head_dim,
                            paths_stream_t stream);
/* The last decoder layer is read at token 0 only (model/aggregator.py:75): single-query attention of the TRAINING path, keys split
 * over workgroups (csrc/attn_token0.hip).  a0 / da0 [B, H*32] = attention output of token 0 and its gradient, lse0 [B, H] (log2
 * domain, un-dropped softmax), dropout p on the probabilities (mask element ((b*H + h)*T + 0)*T + key of site drop_key; p = 0: none);
 * ws: paths_attention_token0_workspace(B, T, H) floats.  The backward writes dk / dv of every valid key and dq of row 0 into dqkv
 * [B, T, 3*H*32] (zero on entry). */
int64_t paths_attention_token0_workspace(int B, int T, int H);
int paths_attention_token0_any(const float* qkv, int64_t ld, const int64_t* num_ims, float* a0, float* ws, int B, int T, int H, int head_dim,
                               float qscale, paths_stream_t stream);      /* inference form for any head_dim on the token-major in_proj output */
int paths_attention_token0_fwd(const float* q, const float* k, const float* v, const int64_t* num_ims, float* a0, float* lse0, float* ws,
                               int B, int T, int H, int head_dim, uint64_t drop_key, float drop_p, paths_stream_t stream);
int paths_attention_token0_bwd(const float* q, const float* k, const float* v, const float* a0, const float* da0, const float* lse0,
                               const int64_t* num_ims, float* dqkv, float* ws, int B, int T, int H, int head_dim, uint64_t drop_key,
                               float drop_p, paths_stream_t stream);
/* Export of the special token's attention (interpretability side path, csrc/attn_token0.hip; what nn.MultiheadAttention returns
 * with need_weights=True, row of the special token): for one decoder layer with input rows x [B, T, d] and its TRUE in_proj_weight
 * [3d, d] / in_proj_bias [3d], per slide b and head h the softmax of q_h . k_t / sqrt(d/H) over the valid tokens t < num_ims[b] + 1
 * (num_ims clamped to [0, T-1]; padding rows are never read).  attn_patch[b*patch_ld + h*(T-1) + j] = weight of patch j (exactly 0
 * for j >= num_ims[b]), attn_self[b*self_ld + h] = weight of the special token on itself.  special_last = 0: special token at row 0,
 * patch j at row j + 1 (the reference's order); 1: patch j at row j, special token at row num_ims[b] (paths_importance_qkv_x6's
 * order).  Any d % H == 0 with d % 4 == 0, d <= 2048.  fp32, deterministic.  ws: paths_token0_attention_workspace(B, T, d, H) floats. */
int64_t paths_token0_attention_workspace(int B, int T, int d, int H);
int paths_token0_attention(const float* x, const int64_t* num_ims, const float* in_proj_weight, const float* in_proj_bias, float* attn_patch,
                           int64_t patch_ld, float* attn_self, int64_t self_ld, float* ws, int B, int T, int d, int H, int special_last,
                           paths_stream_t stream);
/* Attention rollout of the special token (Abnar & Zuidema 2020; interpretability side path, csrc/attn_rollout.hip): with A_l^h the
 * softmax attention of layer l, head h over the valid tokens (T x T), r = e_s^T (0.5 mean_h A_{L-1}^h + 0.5 I) ... (0.5 mean_h A_0^h + 0.5 I).
 * prepare: layer l's Q (scaled) / K rows and per-row softmax statistics from its input rows x [B, T, d] and TRUE in_proj [3d, d] / [3d]
 * (token orders and num_ims clamping as paths_token0_attention) into ws (paths_attention_rollout_workspace floats per layer; rows in
 * canonical order: 0 = special token, 1 + j = patch j).  seed: r [B][T] (canonical) = 0.5 e_s + 0.5 mean_h of the last layer's
 * token-0 attention (paths_token0_attention's layout).  step: r_out = 0.5 r_in + 0.5 mean_h(r_in^T A^h) through a prepared layer.
 * seed / step with r / r_out == NULL write the rollout itself: rollout[b * rollout_ld + j] (patch j, 0 for j >= num_ims[b]),
 * rollout_self[b].  Any d % H == 0 with d % 4 == 0, d <= 2048.  fp32 (f32-input MFMA), deterministic, no T x T buffer. */
int64_t paths_attention_rollout_workspace(int B, int T, int d, int H);
int paths_attention_rollout_prepare(const float* x, const int64_t* num_ims, const float* in_proj_weight, const float* in_proj_bias, float* ws,
                                    int B, int T, int d, int H, int special_last, paths_stream_t stream);
int paths_attention_rollout_seed(const float* attn_patch, int64_t patch_ld, const float* attn_self, int64_t self_ld, const int64_t* num_ims,
                                 float* r, float* rollout, int64_t rollout_ld, float* rollout_self, int B, int T, int H, paths_stream_t stream);
int paths_attention_rollout_step(const float* ws, const int64_t* num_ims, const float* r_in, float* r_out, float* rollout, int64_t rollout_ld,
                                 float* rollout_self, int B, int T, int d, int H, paths_stream_t stream);
/* Gradient-weighted attention relevance of the special token (Chefer, Gur & Wolf 2021; attribution side path of the backward pass,
 * csrc/attn_relevance.hip): with A_l^h the softmax attention of layer l, head h over the valid tokens (row 0 = special
 * token) and gradA_l^h[i][j] = dO_i^h . V_j^h its gradient, Abar_l = mean_h (A_l^h * gradA_l^h)^+ and
 * r = e_s^T (I + Abar_{L-1}) ... (I + Abar_0).
 * Operands of both calls: q / k / v element (b, h, t, e) at base + b*sb + h*sh + t*st + e (floats; strides multiples of 4, bases
 * 16-byte aligned): head-major [B, H, T, hd] with pre-scaled q and qscale = 1, or the token-major qkv [B, T, 3 di] with bases at
 * 0 / di / 2 di and the qscale of paths_attention_bwd_any; scores are qscale * q . k in the log2 domain.  head_dim 16 / 32 / 48 / 64,
 * H the true head count.  num_ims is clamped to [0, T-1] on the device, rows past it are never read, and a slide with num_ims = 0
 * keeps r = e_s (seed) / r_in (step).
 * seed (the last layer, read at token 0): r[b][j] = [j == 0] + 1/H sum_h max(0, p * (da0^h . v_j^h)), p = exp2(qscale q_0 . k_j -
 * lse0) from the saved statistic; da0 [B][da0_ld] with head h at columns [h*hd, (h+1)*hd), lse0 element (b, h) at b*lse0_sb + h*lse0_sh.
 * step (a full layer): r_out[b][j] = r_in[b][j] + 1/H sum_h sum_i r_in[b][i] max(0, exp2(qscale q_i . k_j - lse[b][h][i]) * (dO_i^h . v_j^h));
 * d_o [B][T][ld_o] with head h at columns [h*hd, (h+1)*hd), lse [B][H][T]; r_out must not be r_in.  Both products on the f32-input
 * MFMA, no T x T buffer, no atomics: reruns are bit-identical.
 * r / r_out [B][T] (0 past num_ims); NULL: write the outputs instead: relevance[b * relevance_ld + j] (patch j = row 1 + j, exactly 0
 * for j >= num_ims[b]; may be NULL when T = 1), relevance_self[b]. */
int paths_attention_relevance_seed(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, float qscale,
                                   const float* da0, int64_t da0_ld, const float* lse0, int64_t lse0_sb, int64_t lse0_sh,
                                   const int64_t* num_ims, float* r, float* relevance, int64_t relevance_ld, float* relevance_self, int B,
                                   int T, int H, int head_dim, paths_stream_t stream);
int paths_attention_relevance_step(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, float qscale,
                                   const float* d_o, int64_t ld_o, const float* lse, const int64_t* num_ims, const float* r_in, float* r_out,
                                   float* relevance, int64_t relevance_ld, float* relevance_self, int B, int T, int H, int head_dim,
                                   paths_stream_t stream);

/* Generic out = act(a W^T + b) on the fp32 matrix cores (W rows zero-padded to Npad, a multiple of 128). */
int paths_linear_f32(const float* a, int64_t lda, const float* w, const float* b, float* out, int64_t ldo,
                     int M, int N, int Npad, int K, int act, paths_stream_t stream);

/* Masked multi-head self-attention, flash style (nn.MultiheadAttention inside nn.TransformerDecoderLayer as
 * called at reference model/aggregator.py:70-72, key mask utils.py:97-103).
 *   q,k,v [B,H,T,32] head-major, q pre-scaled by log2(e)/sqrt(32); o [B,T,H*32]; valid keys = num_ims[b]+1.
 *   max_queries > 0 restricts the computed query rows to [0, max_queries) (the last decoder layer is read at
 *   token 0 only, reference model/aggregator.py:75); 0 = all T rows. */
int paths_attention_f32(const float* q, const float* k, const float* v, float* o, float* lse, const int64_t* num_ims,
                        int B, int T, int H, int head_dim, int max_queries, paths_stream_t stream);

/* paths_attention_f32 on the 16-bit matrix cores with fp32 accuracy (csrc/attn_x6.hip): q, k, v are first re-written as
 * split operands in MFMA-fragment order (planes = 3: exact bf16 hi|mid|lo, 6 MFMAs per product block; planes = 2: fp16 hi|lo,
 * 3 MFMAs, |q|, |k|, |v| < 65504; workspace of paths_attention_x6_workspace(B, T, H, head_dim, planes) bytes, caller-owned),
 * then S^T = K Q^T and O^T += V^T P^T run with fp32 accumulation; P is split in registers.
 * Same arguments and results (to fp32 rounding) as paths_attention_f32. */
int64_t paths_attention_x6_workspace(int B, int T, int H, int head_dim, int planes);
int paths_attention_x6(const float* q, const float* k, const float* v, float* o, float* lse, const int64_t* num_ims,
                       int B, int T, int H, int head_dim, int max_queries, void* workspace, int planes, int images_ready,
                       paths_stream_t stream);
/* images_ready != 0 (planes = 2): the workspace already holds the operand images (paths_token_layer_h3 wrote them through its
 * qkv_images argument); q, k, v are not read and the re-write launch is skipped. */

/* Token-row chain of one post-LN decoder layer with empty memory + the next in_proj (same call site):
 *   do_post: x_out = norm3(x' + ffn(x')), x' = norm2(norm1(x_in + out_proj(attn)) + cross_attn_bias)
 *   do_qkv : q,k,v = in_proj(x)  (x = x_out if do_post else x_in) written head-major, q scaled by qscale.
 *   max_tokens > 0 restricts the processed token rows to [0, max_tokens) (last layer); 0 = all T rows. */
int paths_token_layer_f32(const float* x_in, const float* attn, float* x_out,
                          const float* wo, const float* bo, const float* ln1g, const float* ln1b, const float* cab,
                          const float* ln2g, const float* ln2b, const float* w1, const float* b1, const float* w2,
                          const float* b2, const float* ln3g, const float* ln3b, const float* wqkv, const float* bqkv,
                          float* q, float* k, float* v, const int64_t* num_ims, int B, int T, int d, int H,
                          int do_post, int do_qkv, int skip_padding, float qscale, float eps, int max_tokens,
                          paths_stream_t stream);

/* paths_token_layer_f32 on the fp16 matrix cores with fp32 accuracy (csrc/tlayer_h3.hip; two-plane operand split as in the
 * planes = 2 GEMMs, 3 x v_mfma_f32_16x16x32_f16 per product block, activations split in registers).  Weights are passed as
 * images built once per weight version by paths_tlayer_pack_h3: part 0 = (out_proj, linear1, linear2) of THIS layer with
 * power-of-two scales (s_wo, s_w1, s_w2), part 1 = in_proj of the NEXT layer with s_wqkv (max|w| * scale < 65504).
 * Same arguments otherwise, same results to fp32 rounding. */
int64_t paths_tlayer_h3_image_bytes(int part);
int paths_tlayer_pack_h3(int part, const float* wa, const float* wb, const float* wc, float s_a, float s_b, float s_c, void* out,
                         paths_stream_t stream);
int paths_token_layer_h3(const float* x_in, const float* attn, float* x_out, const void* w_post, const void* w_qkv,
                         const float* bo, const float* ln1g, const float* ln1b, const float* cab, const float* ln2g, const float* ln2b,
                         const float* b1, const float* b2, const float* ln3g, const float* ln3b, const float* bqkv,
                         float s_wo, float s_w1, float s_w2, float s_wqkv,
                         float* q, float* k, float* v, const int64_t* num_ims, int B, int T, int d, int H,
                         int do_post, int do_qkv, int skip_padding, float qscale, float eps, int max_tokens, void* qkv_images,
                         paths_stream_t stream);
/* qkv_images (optional, max_tokens = 0): a paths_attention_x6_workspace(B, T, H, 32, 2) buffer; the in_proj outputs are written
 * as the two-plane operand images of paths_attention_x6 (masked keys zeroed) instead of fp32 q, k, v (which may then be null). */

/* paths_token_layer_h3 in WEIGHT-STATIONARY form (csrc/tlayer_ws.hip; reference model/aggregator.py:25-33, 70-72 = torch's post-LN
 * TransformerDecoderLayer after the self-attention, and the next layer's in_proj).  A workgroup = 4 waves = 64 tokens; wave w owns a
 * quarter of every product's output features for all 64 tokens, its weight fragments stream L2 -> registers (never through LDS),
 * activations cross LDS as the fp16 hi | lo B-operand fragments of the next product, LayerNorm statistics as (mean, M2) pairs.
 * w_post / w_qkv: paths_tlayer_pack_ws images (part 0 = out_proj, linear1, linear2 of THIS layer; part 1 = in_proj of the NEXT layer)
 * with their power-of-two scales.  attn: fp32 [B,T,d], or attn_img: the fragment image written by paths_attention_h3_img.
 * qkv_images: a paths_attention_x6_workspace(B, T, 4, 32, 2) buffer that receives the attention operand images (masked keys zeroed).
 * zero_words (optional, do_post): n_zero <= 256 int32 words set to 0 by the launch (arrival counters of paths_token0_tail_ws). */
int64_t paths_tlayer_ws_image_bytes(int part, int d);
int paths_tlayer_pack_ws(int part, const float* wa, const float* wb, const float* wc, float s_a, float s_b, float s_c, void* out, int d,
                         paths_stream_t stream);
int paths_token_layer_ws(const float* x_in, const float* attn, const void* attn_img, float* x_out, const void* w_post, const void* w_qkv,
                         const float* bo, const float* ln1g, const float* ln1b, const float* cab, const float* ln2g, const float* ln2b,
                         const float* b1, const float* b2, const float* ln3g, const float* ln3b, const float* bqkv,
                         float s_wo, float s_w1, float s_w2, float s_wqkv, void* qkv_images, const int64_t* num_ims,
                         int B, int T, int d, int H, int do_post, int do_qkv, int skip_padding, float qscale, float eps,
                         int* zero_words, int n_zero, paths_stream_t stream);
/* The same kernel instantiated at trans_dim 192 (the reference's dataclass default, config.py:30; any head count) with the in_proj result
 * as fp32 token-major rows qkv_rows [B*T][ld_qkv] = [q | k | v] (q UNscaled: the operand of the shape-generic attention kernels)
 * instead of the head_dim-32 fragment images; the attention output enters as fp32 rows.  do_post and / or do_qkv as above. */
int paths_token_layer_ws_rows(const float* x_in, const float* attn, float* x_out, const void* w_post, const void* w_qkv,
                              const float* bo, const float* ln1g, const float* ln1b, const float* cab, const float* ln2g, const float* ln2b,
                              const float* b1, const float* b2, const float* ln3g, const float* ln3b, const float* bqkv,
                              float s_wo, float s_w1, float s_w2, float s_wqkv, float* qkv_rows, int64_t ld_qkv, const int64_t* num_ims,
                              int B, int T, int d, int do_post, int do_qkv, int skip_padding, float eps, paths_stream_t stream);
/* paths_attention_x6 (planes = 2, operand images already in `workspace`) with the output written as the out_proj operand image of
 * paths_token_layer_ws: B * ceil(T/64) * 64 * H * 32 * 4 bytes, [slide][64-token group][head][16-token tile][plane][64 lanes][16 B]. */
int paths_attention_h3_img(void* o_img, const int64_t* num_ims, int B, int T, int H, int head_dim, void* workspace, paths_stream_t stream);

/* paths_token0_tail WITHOUT the last layer's K / V projections, in ONE launch (csrc/token0_ws.hip; reference model/aggregator.py:70-75
 * for the final layer, model/paths.py:130-139).  With one query per head the projections fold into the query and the output:
 * score_h,t = (Wk_h^T q_h) . x_t + const, o_h = Wv_h (sum_t p_h,t x_t) + bv_h, so the launch only reads the layer's INPUT rows
 * x1 [B,T,128].  img: image built once per weight version by paths_token0_pack_ws (A_h = c Wk_h^T Wq_h, a0_h = c Wk_h^T bq_h and
 * 16-byte-transposed Wv, Wo, W1, W2; qscale c = log2(e)/sqrt(head_dim)); bv = in_proj_bias + 2 d.  Workgroups = (token split, head)
 * pairs per slide; each publishes a (max, sum, z[128]) partial, the LAST arriver of a slide (agent-scope release / acquire around an
 * arrival ticket) runs the row chain - or, when all workgroups of the launch fit the chip at once (<= 192), the DISTRIBUTED form:
 * every workgroup pushes its partial through its head's Wv / Wo slices before the ticket and carries a slice of the feed-forward
 * after a flag hop, so that no CU pulls more than ~100 KB of weights.  partials: paths_token0_ws_partials(B, T) floats of scratch;
 * counters: 3 B int32 words, zero on entry, left zero; status (optional): bit 4 set if a bounded hand-off wait gave up.
 * Exact fp32 FMA chains.
 * Widths: trans_dim d = 128 (both forms) and d = 192, the reference's dataclass default (config.py:30; distributed form only, 4 heads
 * of 48: 768 threads per workgroup, x1 [B,T,192]) - the _d entry points take d, the ones without it are the d = 128 forms kept for
 * existing callers.  paths_token0_ws_supported(B, T, d, H): 1 if paths_token0_tail_ws can run the shape (at 192: while the
 * distributed launch fits the chip, B <= 24 on an MI355X, T > 128), else 0 - the caller then takes the generic launches. */
int64_t paths_token0_ws_image_bytes(void);
int64_t paths_token0_ws_image_bytes_d(int d);
int64_t paths_token0_ws_partials(int B, int T);
int64_t paths_token0_ws_partials_d(int B, int T, int d);
int paths_token0_ws_supported(int B, int T, int d, int H);
int paths_token0_pack_ws(const float* wqkv, const float* bqkv, const float* wo, const float* bo, const float* w1, const float* w2, float qscale,
                         void* out, paths_stream_t stream);
int paths_token0_pack_ws_d(const float* wqkv, const float* bqkv, const float* wo, const float* bo, const float* w1, const float* w2, float qscale,
                           int d, void* out, paths_stream_t stream);
int paths_token0_tail_ws(const float* x1, const int64_t* num_ims, const void* img, const float* bv, const float* bo,
                         const float* ln1g, const float* ln1b, const float* cab, const float* ln2g, const float* ln2b,
                         const float* b1, const float* b2, const float* ln3g, const float* ln3b, const float* lnfg, const float* lnfb,
                         const float* ctx_prev, int64_t ctx_stride, const float* ctx_all, int ctx_depth,
                         const float* wcls, const float* bcls, int num_logits, int cls_in,
                         float* ctx_out, float* logits, float* partials, int* counters, int* status, int B, int T, int d, int H,
                         float eps, float eps_final, int special_last /* 1: the special token is row num_ims[b] (paths_importance_qkv_x6's
                         token order) instead of row 0 */, paths_stream_t stream);

/* ---- shape-generic kernels (csrc/generic.hip): any trans_dim (multiple of 32, <= 1024), head_dim in {16, 32, 48, 64}, any
 * importance_mlp_hidden_dim - e.g. the reference's dataclass defaults trans_dim 192 / 4 heads (config.py:30-36).  With
 * paths_gemm_nt_f32 for the products they evaluate model/paths.py:95-98,119-139 and model/aggregator.py:37-76 in exact fp32; the
 * shipped 128 / 4 / 128 geometry runs on the specialised kernels above instead.
 *   paths_attention_any   softmax(q k^T / sqrt(hd)) v, keys >= num_ims[b] + 1 masked; qkv [B*T, 3 d] token-major (in_proj output),
 *                         qscale = log2(e) / sqrt(head_dim), o [B, T, d]; max_queries > 0: only queries [0, max_queries)
 *   paths_layernorm_rows  y = LayerNorm(x (+ add [d])) * gamma + beta per row (row strides ldx / ldy)
 *   paths_importance_rows importance[m] = valid ? sigmoid(hid[m] . w2 + b2) : 0 from hid = relu(Y W1^T + b1)  (utils.py:106-115)
 *   paths_tokens_assemble tokens[b, 0] = special, tokens[b, 1 + n] = alpha P[b n] + bp + PE  (aggregator.py:37-65, utils.py:16-23,47-67)
 *   paths_final_head_any  paths_final_head for any trans_dim */
int paths_attention_any(const float* qkv, int64_t ld, float* o, const int64_t* num_ims, int B, int T, int H, int head_dim, float qscale,
                        int max_queries, paths_stream_t stream);
/* The same attention on the 16-bit matrix cores with fp32-accurate operands (csrc/attn_h3_any.hip: two fp16 planes per operand, three
 * MFMAs per product block - the arithmetic of the tuned head_dim-32 kernel - for head_dim 16 / 32 / 48 / 64); all queries;
 * workspace: paths_attention_h3_any_workspace(B, T, H, head_dim) bytes. */
int64_t paths_attention_h3_any_workspace(int B, int T, int H, int head_dim);
int paths_attention_h3_any(const float* qkv, int64_t ld, float* o, const int64_t* num_ims, int B, int T, int H, int head_dim, float qscale,
                           void* workspace, paths_stream_t stream);
/* ... on operand images already in the workspace (written by paths_token_layer_ws with d = 192, do_qkv only: head_dim 48, q scaled
 * there; or head_dim 32): no prep launch. */
int paths_attention_h3_any_img(float* o, const int64_t* num_ims, int B, int T, int H, int head_dim, void* workspace, paths_stream_t stream);
int paths_layernorm_rows(const float* x, int64_t ldx, const float* add, const float* gamma, const float* beta, float* y, int64_t ldy,
                         int64_t rows, int d, float eps, paths_stream_t stream);
int paths_layernorm2_rows(const float* x, int64_t ldx, const float* g1, const float* b1, const float* add, const float* g2, const float* b2,
                          float* y, int64_t ldy, int64_t rows, int d, float eps, paths_stream_t stream);   /* LN2(LN1(x) + add) in one pass */
int paths_importance_rows(const float* hid, int64_t ldh, const float* w2, const float* b2, const int64_t* num_ims, int rows_per_slide,
                          int64_t M, int Hi, float* importance, int relu /* 1: hid holds the pre-activation, relu applied here */, paths_stream_t stream);
int paths_tokens_assemble(const float* P, int64_t ldp, const float* importance, int imp_mul, const float* bp, const float* special,
                          const float* div_term, const int64_t* locs, int rows_per_slide, int patch_size, int pe_mode, int d, int B,
                          float* tokens, paths_stream_t stream);
/* The importance-rows and tokens-assemble launches (above) as ONE launch over the rows of the [W1 ; Wp] product (csrc/generic.hip; reference
 * model/paths.py:95-98,119-124, model/aggregator.py:37-65, utils.py:16-23,47-67): hid [M, ldh] holds the importance MLP's hidden
 * pre-activations (Hi columns) and the projection (d columns) of every patch row; writes importance [M] (0 for padded rows) and
 * tokens [B, rows_per_slide + 1, d] (special token first; padded rows bp + PE for either imp_mul: their projection is not read,
 * where paths_tokens_assemble and the paths_importance_proj* entry points with imp_mul = 0 add it like any row's).  The positional encoding is read from pe_table
 * (the table built by paths_pe_table for this pe_mode, d and pe_rows): same values as the sin / cos calls of the tokens-assemble launch. */
int paths_importance_tokens_rows(const float* hid, int64_t ldh, const float* w2, const float* b2, const int64_t* num_ims, int rows_per_slide,
                                 int64_t M, int Hi, float* importance, int relu, int imp_mul, const float* bp, const float* special,
                                 const float* pe_table, int pe_rows, const int64_t* locs, int patch_size, int pe_mode, int d, float* tokens,
                                 paths_stream_t stream);
int paths_final_head_any(const float* x, int64_t slide_stride, const float* lng, const float* lnb, const float* ctx_prev, int64_t ctx_stride,
                         const float* ctx_all, int ctx_depth, const float* wcls, const float* bcls, int num_logits, int cls_in,
                         float* ctx_out, float* logits, int B, int d, float eps, paths_stream_t stream);

/* Shape-generic TRAINING kernels (csrc/generic_bwd.hip + the TRAIN form of the generic attention): what autograd applies in the
 * reference train step (train.py:65) to nn.LayerNorm, the importance MLP / scaling / proj_in (model/paths.py:95-98,119-124) and the
 * masked multi-head self-attention incl. its dropout (model/aggregator.py:25-33,70-72), for any trans_dim % 32 == 0 (<= 1024), head_dim
 * 16 / 32 / 48 / 64 and any importance hidden width; the shipped 128 / 4 / 128 geometry trains on the specialised entry points below.
 *   paths_attention_any_train      paths_attention_any + lse [B,H,T] (log2 domain, un-dropped softmax; may be null) + dropout p on the
 *                                  probabilities (mask element ((b*H + h)*T + q)*T + k of site drop_key; p = 0: none)
 *   paths_attention_bwd_any        dqkv [B*T, 3d] = [dq | dk | dv] (token-major, ZERO on entry) from qkv (q unscaled), o, d_o, lse;
 *                                  ws_dsum: B*H*T floats of scratch; max_queries > 0: only those queries carry an output gradient
 *   paths_layernorm_fwd_stats_any  y (may be null), xhat, rstd of LayerNorm(x (+ add [d])) over contiguous [rows, d]
 *   paths_layernorm_bwd_any        dx and dy * xhat
 *   paths_layernorm_bwd_sums_any   dx and one slab [sum dy*xhat | sum dy | sum dx] (3 d floats) per rows_per_block rows
 *   paths_importance_bwd_any       du [M, ldu] = [dhid (Hi) | dP (d) | zeros], da [M], dah [M, Hi] = da * hid
 *   paths_importance_rows_bwd_any  lstm = false (model/paths.py:95-109): the importance MLP's backward through Z = alpha X, any Hi */
int paths_attention_any_train(const float* qkv, int64_t ld, float* o, float* lse, const int64_t* num_ims, int B, int T, int H, int head_dim,
                              float qscale, int max_queries, uint64_t drop_key, float drop_p, paths_stream_t stream);
int paths_attention_bwd_any(const float* qkv, int64_t ld, const float* o, const float* d_o, const float* lse, const int64_t* num_ims,
                            float* dqkv, float* ws_dsum, int B, int T, int H, int head_dim, float qscale, int max_queries,
                            uint64_t drop_key, float drop_p, paths_stream_t stream);
int paths_layernorm_fwd_stats_any(const float* x, const float* add, const float* gamma, const float* beta, float* y, float* xhat,
                                  float* rstd, int64_t rows, int d, float eps, paths_stream_t stream);
int paths_layernorm_bwd_any(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx, float* dyxhat,
                            int64_t rows, int d, paths_stream_t stream);
int paths_layernorm_bwd_sums_any(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx, float* slabs,
                                 int64_t rows, int d, int rows_per_block, paths_stream_t stream);
int paths_importance_rows_bwd_any(const float* dz_rows, const float* x, int D, const float* hid, const float* alpha, const float* w2,
                                  const int64_t* num_ims, int rows_per_slide, int64_t M, int Hi, float* dh, float* da, float* dah,
                                  paths_stream_t stream);
int paths_importance_bwd_any(const float* dtok, const float* pproj, const float* hid, const float* alpha, const float* w2,
                             const int64_t* num_ims, int rows_per_slide, int64_t M, int imp_mul, int Hi, int d, int64_t ldu, float* du,
                             float* da, float* dah, paths_stream_t stream);

/* LAST decoder layer evaluated at token 0 only + decoder.norm + slide-context residual / concat + classifier, one
 * launch (reference model/aggregator.py:70-75 for the final layer, model/paths.py:130-139).  Legal because only
 * out[:, 0] of the final layer is read: it needs K/V of every token (q,k,v as written by paths_token_layer_f32 for
 * that layer) but queries / out_proj / norms / FFN of one row per slide.  x_in = the layer's input activations;
 * ws_partials = scratch of B*H*16*36 floats (split-key attention partials). */
int paths_token0_tail(const float* x_in, const float* q, const float* k, const float* v, const int64_t* num_ims,
                      const float* wo, const float* bo, const float* ln1g, const float* ln1b, const float* cab,
                      const float* ln2g, const float* ln2b, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* ln3g, const float* ln3b, const float* lnfg, const float* lnfb,
                      const float* ctx_prev, int64_t ctx_stride, const float* ctx_all, int ctx_depth,
                      const float* wcls, const float* bcls, int num_logits, int cls_in,
                      float* ctx_out, float* logits, float* ws_partials, int B, int T, int d, int H, float eps,
                      float eps_final, paths_stream_t stream);

/* decoder.norm on token 0, slide-context residual / concat, classifier
 * (reference model/aggregator.py:75, model/paths.py:130-139). */
int paths_final_head(const float* x, int64_t slide_stride, const float* lng, const float* lnb,
                     const float* ctx_prev, int64_t ctx_stride, const float* ctx_all, int ctx_depth,
                     const float* wcls, const float* bcls, int num_logits, int cls_in,
                     float* ctx_out, float* logits, int B, int d, float eps, paths_stream_t stream);

/* Stand-alone wavefront-reduction LayerNorm over rows of width 128 (aten::native_layer_norm). */
int paths_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int d,
                        float eps, paths_stream_t stream);

/* torch.topk(importance[:n], min(n, keep)).indices per slide (reference data_utils/slide.py:294-301).
 * Order: score descending, ties by index ascending.  keep = -1 keeps every patch in original order.
 * "Descending" is the order of the scores' BIT PATTERNS (csrc/rank_key.h), which is the numeric order of all ordinary values, puts
 * +0.0 before -0.0, a NaN with a clear sign bit before +inf and a NaN with the sign bit set after -inf (torch.topk ranks every NaN
 * first: a negative NaN is the one case where the two differ).  Only scores[b, 0:num_ims[b]] are read (ld >= n_max is the row
 * stride); keep_idx[b, keep_count[b]:ldk] is left untouched. */
int paths_topk(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep,
               int* keep_idx, int64_t ldk, int* keep_count, paths_stream_t stream);
/* paths_topk + kept_rows[b, i] = address of row_base[b, keep_idx[b, i], 0] of a row-major [B, slide_rows, row_ld] float table
 * (entries beyond keep_count[b] = zero_row): lets paths_gemm_rows_nt_x6 read the kept parents' rows in place. */
int paths_topk_rows(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep,
                    int* keep_idx, int64_t ldk, int* keep_count, const float* row_base, int64_t row_ld, int64_t slide_rows,
                    int64_t* kept_rows, const float* zero_row, paths_stream_t stream);
/* The same two selections for levels of more than 8,192 patches (csrc/topk_tiled.hip): same parameters, same outputs byte for byte,
 * same key.  The twins above hold all keys of a slide in LDS, which ends at n_max = 8,192; these stream them through a fixed 16-KiB
 * LDS tile, so n_max and ldk go up to PATHS_TOPK_TILED_MAX - the most patches the token-0 attention entries take (65,536 tokens, one of
 * them the special token); past it n^2 rank counting stops being a small share of a level.  n_max <= 8,192 is accepted too (the two
 * families can be compared on one input).  num_ims[b] is clamped to [0, n_max].  Return -1 without launching unless B > 0,
 * 1 <= n_max <= PATHS_TOPK_TILED_MAX, keep is -1 or > 0, (keep < 0 ? n_max : min(keep, n_max)) <= ldk <= PATHS_TOPK_TILED_MAX,
 * ld >= n_max and no required pointer is null; the _rows form also needs row_ld > 0 and slide_rows >= n_max.  One launch each, which
 * carries a pending stop event like the twins' (paths_set_stop_event). */
#define PATHS_TOPK_TILED_MAX 65535
int paths_topk_tiled(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep,
                     int* keep_idx, int64_t ldk, int* keep_count, paths_stream_t stream);
int paths_topk_rows_tiled(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep,
                          int* keep_idx, int64_t ldk, int* keep_count, const float* row_base, int64_t row_ld, int64_t slide_rows,
                          int64_t* kept_rows, const float* zero_row, paths_stream_t stream);

/* 4-child expansion, bounds + background filter, stable compaction (reference data_utils/slide.py:303-331).
 *   mask_ptrs[b] -> uint8 [X*Y] tissue mask of the NEXT level (1 = row sum != 0).  status bit0: a slide
 *   produced zero children (reference fallback slide.py:336-352 needed), bit1: capacity n_next exceeded.
 *   child_pos (optional, [B, 4*ldk]): output row of every candidate child (-1 if dropped), for paths_gather_rows_bwd.
 *   hp_row (optional, [B, n_next]): row b*ldk + i of the kept-parent table for every child (-1 on padding), see paths_lstm_cell.
 *   src_cell is the child's cell x * Y + y in the next grid.  keep_count[b] is clamped to [0, ldk] like in the split form below; a
 *   slide over capacity writes num_out[b] only.  Returns -1 without launching unless ldk > 0 and every pointer but child_pos / hp_row
 *   is non-null. */
int paths_expand_children(const int* keep_idx, int64_t ldk, const int* keep_count, const int64_t* locs, int64_t n_cur,
                          int patch_size, const int* next_x, const int* next_y, const int64_t* mask_ptrs, int B,
                          int64_t n_next, int64_t* num_out, int64_t* locs_out, int64_t* parent_out, int* src_row,
                          int* src_cell, int* status, int* child_pos, int* hp_row, paths_stream_t stream);

/* paths_expand_children split around the caller, for slides whose next-level features are encoded on demand (no tissue mask of the next
 * grid exists: whether a cell is tissue is known only once the caller has supplied its row; reference RawSlide.recurse,
 * data_utils/slide.py:173-198).  One workgroup per slide each.
 *
 * paths_candidate_children - the first half: the four children of every kept patch in the block order of slide.py:305-315
 *   ((2x,2y) | (2x,2y+1) | (2x+1,2y) | (2x+1,2y+1), each block in top-K order), those inside the next grid (next_x / next_y [B]),
 *   compacted stably.  cand_count [B]; cand_cells [B, 4*ldk, 2]: int64 CELL coordinates (the cells to encode); cand_slot [B, 4*ldk]:
 *   the kept slot i of the parent.  Entries at and beyond cand_count[b] are -1 in both tables.
 * paths_admit_children - the second half: cand_mask [B, 4*ldk] (1 = the row supplied for that candidate has fp32 sum != 0, i.e.
 *   paths_tissue_mask_absmax[_h16] over the candidate rows as a grid of B * 4*ldk cells) selects the admitted candidates, compacted
 *   stably; num_out, locs_out (pixel coordinates), parent_out, src_row (= keep_idx[b, slot]), hp_row (= b*ldk + slot, optional),
 *   child_pos (optional, indexed like paths_expand_children's) and the zeroed padding tail are what paths_expand_children writes;
 *   src_cell is the candidate's index in the slide's candidate rows (grid_ptrs[b] of paths_gather_rows* = the address of slide b's
 *   first candidate row).  A candidate whose slot is not in [0, keep_count[b]) is never admitted.  status bit0: a slide without an
 *   admitted child, bit1: n_next exceeded (that slide then writes num_out[b] only). */
int paths_candidate_children(const int* keep_idx, int64_t ldk, const int* keep_count, const int64_t* locs, int64_t n_cur,
                             int patch_size, const int* next_x, const int* next_y, int B, int* cand_count, int64_t* cand_cells,
                             int* cand_slot, paths_stream_t stream);
int paths_admit_children(const int* cand_count, const int64_t* cand_cells, const int* cand_slot, const uint8_t* cand_mask,
                         const int* keep_idx, int64_t ldk, const int* keep_count, int patch_size, int B, int64_t n_next,
                         int64_t* num_out, int64_t* locs_out, int64_t* parent_out, int* src_row, int* src_cell, int* status,
                         int* child_pos, int* hp_row, paths_stream_t stream);

/* The row cache of on-demand slides that keep what their encoder produced (paths_amd/data_utils/slide.py:CachedOnDemandSlide;
 * csrc/row_cache.hip; no reference equivalent - RawSlide.recurse encodes every visit anew).  Per slide b and level the cache
 * is a cell index (int32 [X, Y]: the row of a cell in the store, or -1) and a row store [capacity[b], D] with count[b] rows in use.
 * Every per-slide argument is a DEVICE table [B]: int64 addresses (cells_ptrs: the request, int64 [n[b], 2] cell coordinates; index_ptrs;
 * enc_ptrs: the rows the caller's encoder returned for the misses, [miss_count[b], D], never dereferenced without a miss; store_ptrs),
 * int64 n / count / capacity, int32 gx / gy (the level's grid).  n[b] is clamped to [0, n_max]; n[b] = 0 is a slide without a request.
 * Rows are D fp32 (paths_cache_fill) or fp16 (_h16) elements; store, encoder rows and out are 16-byte aligned.  One launch each for the
 * whole batch; integers and copies only, no atomics, no workspace: a rerun on the same inputs writes the same bytes.  Both return -1
 * and launch nothing unless B > 0, n_max > 0, D is a positive multiple of 4 and no pointer is null.  Contract: tests/cache_ref.py.
 *
 * paths_cache_probe - one workgroup per slide, the request in chunks of PATHS_CACHE_PROBE_CHUNK cells.  For i < n[b]:
 *   src[b, i] = the store row (>= 0) of a cell the index holds;  -1 - j for the j-th cell it does not hold, in request order;
 *   PATHS_CACHE_SRC_NONE for a cell outside the gx[b] x gy[b] grid (it reads as a zero row and is not a miss).
 *   miss_count[b] = the number of misses m_b, miss_cells[b, 0:m_b] = their coordinates in request order (what to hand the encoder),
 *   status[b] = 1 if the request names a cell outside the grid, else 0.  src [B, n_max] beyond n[b] and miss_cells [B, n_max, 2] beyond
 *   m_b are left untouched; nothing is read beyond n[b].  D is the cache's row width (checked only).
 * paths_cache_fill / _h16 - one wave per row of out [B, n_max, D], the buffer the recursion reads (a hit row moves once).  For i < n[b]:
 *   src >= 0 (and < count[b]):  out[b, i] = store_b[src];
 *   src = -1 - j (j < miss_count[b]):  out[b, i] = enc_b[j]; if count[b] + j < capacity[b] also store_b[count[b] + j] = enc_b[j] and
 *   index_b[cell i] = count[b] + j - the first capacity[b] - count[b] misses in request order are kept, the rest pass through;
 *   anything else (PATHS_CACHE_SRC_NONE, a src no store row or encoder row stands behind): out[b, i] = +0.
 *   Rows n[b] <= i < n_max of out are +0.  count itself is the caller's to advance (by min(m_b, capacity[b] - count[b])).
 *   A request must not name a cell twice (the recursion's candidates never do): both copies would be misses with rows of their own,
 *   and which of them the index then names is not defined.  The fill of a probe's src must follow it with the index unchanged.
 * Undefined memory: src / miss_cells / out on entry: never read; store rows at and beyond count[b]: never read. */
#define PATHS_CACHE_PROBE_CHUNK 1024
#define PATHS_CACHE_SRC_NONE (-2147483647 - 1)
int paths_cache_probe(const int64_t* cells_ptrs, const int64_t* n, const int64_t* index_ptrs, const int* gx, const int* gy, int B, int n_max,
                      int D, int* src, int* miss_count, int64_t* miss_cells, int* status, paths_stream_t stream);
int paths_cache_fill(const int64_t* cells_ptrs, const int64_t* n, const int* src, const int* miss_count, const int64_t* enc_ptrs,
                     const int64_t* store_ptrs, const int64_t* count, const int64_t* capacity, const int64_t* index_ptrs, const int* gx,
                     const int* gy, int B, int n_max, int D, float* out, paths_stream_t stream);
int paths_cache_fill_h16(const int64_t* cells_ptrs, const int64_t* n, const int* src, const int* miss_count, const int64_t* enc_ptrs,
                         const int64_t* store_ptrs, const int64_t* count, const int64_t* capacity, const int64_t* index_ptrs, const int* gx,
                         const int* gy, int B, int n_max, int D, void* out, paths_stream_t stream);

/* From decoded pixels to encoder input and back to feature rows (paths_amd/pixels.py; csrc/tiles.hip; the tissue decision,
 * to_tensor / Normalize and the scatter of reference preprocess/preprocess.py:27-110 and data_utils/slide.py:80-161).  Contract:
 * tests/tiles_ref.py, bit for bit.  Integer and table work only: no float arithmetic but the one cast of paths_scatter_rows, no global
 * atomics; a rerun on the same inputs writes the same bytes.
 *
 * Pixels are uint8 RGB with pixel stride 3; grey g = (4899 R + 9617 G + 1868 B + 8192) >> 14 (OpenCV's 8-bit RGB2GRAY).
 * IMAGES are named by a DEVICE table [n_images][4] int64 = (address of the first byte, row stride in bytes, rows, cols); TILES by a
 * DEVICE table [n][2] int64 = (address of the tile's first byte, its row stride in bytes): tile k is the P x P window whose row r is the
 * 3 P bytes at address + r * stride - a [n, P, P, 3] batch and windows into a resident image alike.  Addresses and strides are
 * multiples of 16, a stride is at least the row's bytes; P % 16 == 0, 16 <= P <= PATHS_TILE_MAX_P, n <= PATHS_TILES_MAX.  What the host
 * can see is refused with -1 before any launch; a table entry that breaks the rule is never followed: the image counts nothing
 * and paths_grey_histogram sets *status, the tile gets count -1 and flag 0 (paths_tile_compact reports it in *status) and reads as
 * zero bytes in paths_tiles_to_input.
 *
 * paths_grey_histogram - counts [256] int64 = the number of pixels of every grey value over all images, jointly.  PATHS_HIST_BLOCKS
 *   workgroups per image keep their counts in LDS (integer adds: the order does not matter) and write them to partials
 *   (paths_grey_histogram_workspace(n_images) bytes); a second launch of one workgroup sums the partials in a fixed order.
 *   n_images in [1, PATHS_HIST_MAX_IMAGES]; an image holds fewer than 2^31 pixels.  *status (int32) = 1 if any image entry was
 *   refused (misaligned address or stride, a stride shorter than the row, no or too many pixels), else 0.
 * paths_tile_tissue - counts[k] int32 = the number of lattice pixels (i s + s / 2, j s + s / 2), 0 <= i, j < P / s, s = stride, P % s == 0,
 *   with g < threshold (strict; threshold in [0, 256]); flags[k] uint8 = counts[k] >= pass_count (the host's integer form of
 *   count / size > tissue_threshold; 0 <= pass_count <= (P / s)^2 + 1).  One workgroup per tile.
 * paths_tile_compact - one workgroup: order[0 .. m) int32 = the tiles with a set flag in request order, *m = their number, slot[k] =
 *   the position of tile k in order, or -1; *status = 1 if any counts[k] < 0 (a refused table entry), else 0.
 * paths_tiles_to_input - out [count, 3, P, P] of elem_bytes-wide elements (2: fp16 or bf16, 4: fp32): out[i, c, r, x] =
 *   table[c * 256 + byte c of pixel (r, x) of tile order[first + i]], table [3][256] of the same element type (held in LDS; a copy of
 *   bits, so the result is what indexing the table gives).  A thread owns 16 consecutive pixels of a row: three 16-byte loads, then
 *   16-byte stores per channel plane.  An order entry outside [0, n) reads as zero bytes.  count >= 1, first >= 0.
 * paths_scatter_rows - out [n, dim] fp32 (out_f16 = 0) or fp16 (1): row k = enc[slot[k]] (enc [m, dim] fp32 or fp16 (enc_f16), cast once,
 *   round to nearest even) when 0 <= slot[k] < m, else +0.  dim % 4 == 0; enc (may be NULL when m = 0) and out 16-byte aligned; 16-byte
 *   stores (the last 8 bytes of an fp16 output of odd n * dim / 4 apart). */
#define PATHS_TILES_MAX 65536
#define PATHS_TILE_MAX_P 1024
#define PATHS_HIST_BLOCKS 64
#define PATHS_HIST_MAX_IMAGES 1024
int64_t paths_grey_histogram_workspace(int n_images);
int paths_grey_histogram(const int64_t* images, int n_images, uint32_t* partials, int64_t* counts, int* status, paths_stream_t stream);
int paths_tile_tissue(const int64_t* tiles, int n, int P, int stride, int threshold, int pass_count, int* counts, uint8_t* flags,
                      paths_stream_t stream);
int paths_tile_compact(const uint8_t* flags, const int* counts, int n, int* order, int* m, int* slot, int* status, paths_stream_t stream);
int paths_tiles_to_input(const int64_t* tiles, int n, const int* order, int first, int count, int P, const void* table, int elem_bytes,
                         void* out, paths_stream_t stream);
int paths_scatter_rows(const void* enc, int enc_f16, int m, const int* slot, int n, int dim, int out_f16, void* out, paths_stream_t stream);

/* Resize and centre crop in front of the table (csrc/tile_resize.hip; pixels.encoder_input(resize=...); contract
 * tests/resize_ref.py, bit for bit): what Resize(S, bicubic | bilinear) -> CenterCrop(C) -> ToTensor -> Normalize give for a decoded
 * square tile when the resize is Pillow's, as in timm's and torchvision's transforms of PIL images.  out [count, 3, C, C] of
 * elem_bytes-wide elements: out[i, c, r, x] = table[c * 256 + o_c[off + r][off + x]], o the S x S resize of tile order[first + i] and
 * off = int(round((S - C) / 2.0)) (half to even: S = 17, C = 16 gives 0).  Tiles, order, first, count, table and the treatment of an
 * order entry outside [0, n) or a refused tile entry (zero bytes: the output is table[c][0] everywhere) are paths_tiles_to_input's.
 *
 * The resize is Pillow's ImagingResample for 8-bit images, in integers.  bounds [S][2] int32 = (lo, cnt) and coef [S][taps] int32
 * (22 fractional bits; zero at and beyond cnt) are DEVICE tables for one axis - tiles are square, one table serves both -, built by
 * pixels.resize_coefficients.  Horizontal pass first, into a BYTE image: h[r][j] = clip((2^21 + sum_t px[r][lo_j + t] coef_j[t]) >> 22,
 * 0, 255) (arithmetic shift), then o[i][j] = clip((2^21 + sum_t h[lo_i + t][j] coef_i[t]) >> 22, 0, 255), per channel.  The sums are
 * int32 (255 sum|coef| + 2^21 < 2^31 per row) and the products 24-bit multiplies (|coef| < 2^23): the builder of the tables checks both.
 * The host cannot inspect the tables: the kernel clamps cnt into [0, taps] and every source row and column into the window it
 * staged, so whatever they hold it reads only bytes of the tile's P x 3P window and LDS it wrote (the values are then meaningless).
 *
 * Domain: P as above; 16 <= C <= S <= PATHS_RESIZE_MAX, C % 16 == 0 (an output row is whole 16-byte stores); P <= 4 S, so that
 * taps <= PATHS_RESIZE_MAX_TAPS; taps = ceil(f max(P / S, 1)) * 2 + 1 for f = 1 (bilinear) or f = 2 (bicubic).  A workgroup takes one
 * tile and a band of R of the C output rows; it keeps in LDS
 *   768 elem_bytes + 4 (C (taps + 2) + 2 R + R taps) + 3 rows (P + C) bytes, rows = min((R - 1) P / S + taps + 1, P)
 * (the table, the coefficient rows of the cropped columns and of the band, the staged input rows as byte planes and their horizontal
 * results; 2 R and R taps rounded up to multiples of 4).  R is the largest band within 64 KiB (two workgroups per compute unit),
 * divided evenly; if not even R = 1 fits, within 160 KiB; a shape whose R = 1 exceeds that is refused.  Everything outside the domain
 * is refused with -1 before any launch. */
#define PATHS_RESIZE_MAX 1024
#define PATHS_RESIZE_MAX_TAPS 17
int paths_tiles_resize_to_input(const int64_t* tiles, int n, const int* order, int first, int count, int P, int S, int C, const int* bounds,
                                const int* coef, int taps, const void* table, int elem_bytes, void* out, paths_stream_t stream);

/* Rare fallback of reference data_utils/slide.py:336-352 for slides with num_out[b] == 0 after paths_expand_children:
 * continue with every tissue cell of the next grid (every cell if it has no tissue), zero patch context (src_row = -1),
 * parent_inds = cell index.  Other slides are untouched.  status bit1 set if n_next is too small (that slide writes num_out[b]
 * only); rows at and beyond num_out[b] are not rewritten.  Returns -1 without launching if any pointer but hp_row is null. */
int paths_fallback_all_cells(const int* next_x, const int* next_y, const int64_t* mask_ptrs, int patch_size, int B,
                             int64_t n_next, int64_t* num_out, int64_t* locs_out, int64_t* parent_out, int* src_row,
                             int* src_cell, int* status, int* hp_row, paths_stream_t stream);

/* Gather child features from the next-level grids and parent LSTM state (reference slide.py:318,327-331;
 * zero padding of data_utils/dataset.py:216-227 when zero_pad != 0).  state_cur points at the first state column to copy
 * (row stride ld_state_cur), Dp = number of columns copied into state_out [B, n_next, Dp].
 * fts_out may be NULL when row_ptrs [B, n_next] is given: the features are then not copied at all, row_ptrs receives the
 * ADDRESS of every child's feature row inside its resident grid (padding rows: zero_row, D zeros) and the split-operand
 * GEMMs read the rows in place (x_rows / y_rows of paths_lstm_cell_x6 / paths_importance_proj_x6).
 * grid_ptrs [B] may hold pinned, device-mapped HOST addresses (host-resident slides): with fts_out the rows are copied over the host
 * link by this kernel; with row_ptrs alone nothing is read from the grids and paths_stage_rows fetches the rows afterwards. */
int paths_gather_rows(const int64_t* grid_ptrs, const int* src_cell, int D, const float* state_cur, int64_t n_cur,
                      int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                      float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row,
                      paths_stream_t stream);
/* paths_gather_rows over FP16 grids: row_ptrs address fp16 rows, fts_out (optional) receives fp32 copies; zero_row as above. */
int paths_gather_rows_h16(const int64_t* grid_ptrs, const int* src_cell, int D, const float* state_cur, int64_t n_cur,
                          int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                          float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row,
                          paths_stream_t stream);

/* Compact table of the kept parents' rows: out[b*ldk + i] = src[b, keep_idx[b,i], 0:D] (zeros beyond keep_count). */
int paths_gather_kept_rows(const float* src, int64_t n_cur, int64_t ld_src, const int* keep_idx, int64_t ldk, const int* keep_count,
                           int D, int B, float* out, paths_stream_t stream);

/* Backward of the parent-state gather: d_cur[b, keep_idx[i]] = sum over the surviving children of parent i of d_next
 * (d_cur zero-initialised by the caller). */
int paths_gather_rows_bwd(const int* keep_idx, int64_t ldk, const int* keep_count, const int* child_pos, const float* d_next,
                          int64_t n_next, int Dp, float* d_cur, int64_t n_cur, int B, paths_stream_t stream);

/* The once-per-parent form of the TRAINING step (siblings share their parent's h, reference data_utils/slide.py:303-331 +
 * model/interface.py:49-56): paths_sibling_sum adds the rows of the surviving children of every kept parent -
 * dst[b, row(i), 0:width] = sum_children src[b, child, 0:width], row(i) = keep_idx[b, i] or, with keep_idx NULL, the compact slot i
 * (the gradient of the once-per-parent partial pre-activations: dHP = sum of the children's dG) - and paths_scatter_kept_rows puts
 * a compact per-kept-parent table back into the level's rows: dst[b, keep_idx[b, i], 0:width] = src[b, i, 0:width]. */
int paths_sibling_sum(const int* keep_idx, int64_t ldk, const int* keep_count, const int* child_pos, const float* src, int64_t n_src,
                      int64_t ld_src, int width, float* dst, int64_t n_dst, int64_t ld_dst, int B, paths_stream_t stream);
int paths_scatter_kept_rows(const float* src, int64_t ldk, int64_t ld_src, const int* keep_idx, const int* keep_count, float* dst,
                            int64_t n_dst, int64_t ld_dst, int width, int B, paths_stream_t stream);

/* Level-0 batch: every grid cell in row-major order (reference data_utils/slide.py:257-269,362-381).  grid_ptrs [B]: base address of
 * every slide's level-0 grid, device memory or pinned device-mapped host memory (with fts the rows are then copied over the host
 * link; with row_ptrs only their addresses are written, for paths_stage_rows). */
int paths_level0_batch(const int64_t* grid_ptrs, const int* gx, const int* gy, int B, int D, int patch_size, int64_t n0,
                       float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                       const float* zero_row, paths_stream_t stream);
/* paths_level0_batch over FP16 grids (row_ptrs address fp16 rows, fts receives fp32 copies). */
int paths_level0_batch_h16(const int64_t* grid_ptrs, const int* gx, const int* gy, int B, int D, int patch_size, int64_t n0,
                           float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                           const float* zero_row, paths_stream_t stream);

/* Tissue-only (PACKED) slides (paths_amd/data_utils/slide.py: DeviceSlide.pack / from_patches; no reference equivalent - the reference
 * stores background cells as all-zero rows, preprocess/loader.py).  A packed level is rows [n, D] (fp32 or fp16; device memory or
 * pinned device-mapped host memory) behind index: int32 [X*Y] DEVICE table, the row number of a cell or -1 for a cell whose row was
 * all +0.0 and is not stored.
 *
 * paths_gather_rows_packed[_h16] / paths_level0_batch_packed[_h16]: the arguments and results of their twins above with
 * grid_ptrs[b] = the address of slide b's first packed row (never dereferenced for a level without rows) and index_ptrs [B] = the
 * addresses of the slides' index tables.  src_cell stays the cell x * Y + y of the dense grid.  A cell with index -1 reads as the
 * all-zero row it was: zero_row in row_ptrs (required with row_ptrs), zeros in the copy (written whatever zero_pad says: it is a
 * valid row).  State copy, padding rows and zero_pad are those of the twins. */
int paths_gather_rows_packed(const int64_t* grid_ptrs, const int* src_cell, int D, const float* state_cur, int64_t n_cur,
                             int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                             float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row,
                             const int64_t* index_ptrs, paths_stream_t stream);
int paths_gather_rows_packed_h16(const int64_t* grid_ptrs, const int* src_cell, int D, const float* state_cur, int64_t n_cur,
                                 int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                                 float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row,
                                 const int64_t* index_ptrs, paths_stream_t stream);
int paths_level0_batch_packed(const int64_t* grid_ptrs, const int* gx, const int* gy, int B, int D, int patch_size, int64_t n0,
                              float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                              const float* zero_row, const int64_t* index_ptrs, paths_stream_t stream);
int paths_level0_batch_packed_h16(const int64_t* grid_ptrs, const int* gx, const int* gy, int B, int D, int patch_size, int64_t n0,
                                  float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                                  const float* zero_row, const int64_t* index_ptrs, paths_stream_t stream);

/* Packing a dense grid [cells, D] on the device (csrc/pack_rows.hip), three passes on the caller's stream:
 *   paths_pack_flags[_h16]  flags[cell] (uint8) = 1 iff any BIT of the row is set (only all-+0.0 rows give 0; -0.0 is a set bit);
 *   paths_pack_index        index[cell] (int32) = flags[cell] ? number of flagged cells in front of it (row-major) : -1, and *count
 *                           (device int32) = the number of flagged cells.  partials: scratch of paths_pack_index_partials(cells)
 *                           int32.  Integer block sums in a fixed order, no atomics: bit-identical on repeat;
 *   paths_pack_rows[_h16]   rows[index[cell]] = grid[cell] for index[cell] in [0, n_rows); other cells are not read.
 * D % 4 == 0; rows move 16 bytes per lane where the row size and both bases allow, else 8; 1 <= cells < 2^31. */
int paths_pack_flags(const float* grid, int64_t cells, int D, uint8_t* flags, paths_stream_t stream);
int paths_pack_flags_h16(const void* grid, int64_t cells, int D, uint8_t* flags, paths_stream_t stream);
int64_t paths_pack_index_partials(int64_t cells);
int paths_pack_index(const uint8_t* flags, int64_t cells, int* index, int* count, int* partials, paths_stream_t stream);
int paths_pack_rows(const float* grid, int64_t cells, int D, const int* index, int64_t n_rows, float* rows, paths_stream_t stream);
int paths_pack_rows_h16(const void* grid, int64_t cells, int D, const int* index, int64_t n_rows, void* rows, paths_stream_t stream);

/* Row staging for host-resident slides (paths_amd/data_utils/slide.py:HostSlide; the reference gathers rows on the CPU from grids in
 * host RAM, data_utils/slide.py:320-331).  row_ptrs [rows] is an address table written by paths_level0_batch* / paths_gather_rows*
 * whose grid_ptrs were pinned, device-mapped HOST addresses: for every m with row_ptrs[m] != zero_row the row_bytes bytes at
 * row_ptrs[m] (16-byte aligned) are copied over the host link to stage + m * row_bytes and row_ptrs[m] is rewritten to that address;
 * entries equal to zero_row (padding) are neither followed nor changed.  stage: DEVICE buffer of rows * row_bytes bytes, 16-byte
 * aligned.  A byte copy: one entry point for fp32 and fp16 rows.  Each source row is read once; row_bytes % 16 == 0. */
int paths_stage_rows(int64_t* row_ptrs, int64_t rows, int row_bytes, void* stage, const void* zero_row, paths_stream_t stream);

/* Per-patch reductions of the feature gradient (paths_amd/saliency.py:input_gradients; interpretability side path,
 * csrc/saliency_rows.hip).  For every row r of [B * rows_per_slide]: gxi[r] = sum_d dx[r,d] x[r,d] (gradient x input) and
 * gnorm[r] = sqrt(sum_d dx[r,d]^2); rows at or beyond num_ims[b] are not read and get exact zeros in both.  dx / x: fp32 rows with
 * element strides ldd / ldx (multiples of 4, >= D; 16-byte aligned bases); D % 128 == 0.  Fixed summation order per row
 * (bit-reproducible), no workspace, no atomics. */
int paths_saliency_rows(const float* dx, int64_t ldd, const float* x, int64_t ldx, const int64_t* num_ims, int rows_per_slide, int D,
                        int B, float* gxi, float* gnorm, paths_stream_t stream);

/* Row kernels of the attributions taken along the recursion's frozen path (paths_amd/saliency.py:integrated_gradients / smooth_grad;
 * csrc/path_rows.hip).  C chunk members of B slides form B * C virtual slides, virtual slide v = c * B + b.  x: the
 * recorded fp32 rows [B, rows_per_slide, D] with element stride ldx between rows (a multiple of 4, >= D; 16-byte aligned base);
 * D % 128 == 0; base: [D] fp32, 16-byte aligned, or NULL (zero); alpha, sigma, w: DEVICE tables [C] fp32; num_ims: [B].  One
 * wavefront per recorded row, members in ascending c, fixed summation order (bit-reproducible), no workspace, no atomics.
 *
 * paths_path_points: out [C * B, rows_per_slide, D] (contiguous, 16-byte aligned).  For r < num_ims[b]:
 *     t = x[b,r,d] - base[d]                               (base NULL: t = x exactly)
 *     out[v,r,d] = fmaf(alpha[c], t, base[d])  +  sigma[c] * rms(x[b,r,:]) * z(keys[v], r * D + d)
 * (base NULL: the first term is alpha[c] * x), rms = sqrt(sum_d x^2 / D) in the row's fixed order; rows at or beyond num_ims[b] are
 * not read and get exact zeros.  sigma[c] == 0 skips the noise term (no hash is computed): alpha = 1, sigma = 0, base = NULL
 * returns x bit for bit.  keys: DEVICE table [C * B] of 64-bit keys (low word key_lo, high word key_hi); may be NULL when every
 * sigma is 0.  z is a counter-based standard normal draw on csrc/dropout.h's drop_hash, one Box-Muller pair per element pair; with
 * e = r * D + d:
 *     h0 = drop_hash(e & ~1, key_lo, key_hi)     h1 = drop_hash(e | 1, key_lo, key_hi)
 *     u1 = ((h0 >> 8) + 0.5) * 2^-24             u2 = (h1 >> 8) * 2^-24             rad = sqrt(-2 ln u1)
 *     z(even e) = rad * cos(2 pi u2)             z(odd e)  = rad * sin(2 pi u2)
 * |z| <= 5.89.  Nothing is stored: the same (key, e) gives the same draw in any chunking.
 *
 * paths_path_accumulate: dx [C * B, rows_per_slide, D] fp32 with element stride ldd between rows (as ldx).  For r < num_ims[b], in
 * ascending c:
 *     g_c = sum_d dx[v,r,d] * (x[b,r,d] - base[d])          q_c = sum_d dx[v,r,d]^2
 *     acc_gxi[b,r] = (init ? 0 : acc_gxi[b,r]) + w[0] g_0 + w[1] g_1 + ...      (in this order)
 *     acc_sq[b,r]  = (init ? 0 : acc_sq[b,r])  + w[0] q_0 + w[1] q_1 + ...
 * acc_dx [B, rows_per_slide, D] (contiguous, 16-byte aligned; may be NULL): (init ? 0 : acc_dx[b,r,:]) + w[0] dx[0 B + b,r,:] + ...
 * With init, rows at or beyond num_ims[b] are written as exact zeros (in all three); otherwise they are not touched.  x is the
 * un-perturbed recorded row. */
int paths_path_points(const float* x, int64_t ldx, const float* base, const float* alpha, const float* sigma, const uint64_t* keys,
                      const int64_t* num_ims, int rows_per_slide, int D, int B, int C, float* out, paths_stream_t stream);
int paths_path_accumulate(const float* dx, int64_t ldd, const float* x, int64_t ldx, const float* base, const float* w,
                          const int64_t* num_ims, int rows_per_slide, int D, int B, int C, int init, float* acc_gxi, float* acc_sq,
                          float* acc_dx, paths_stream_t stream);

/* Deletion and insertion curves along the frozen path (paths_amd/saliency.py:perturbation_curves; csrc/perturb_rows.hip).
 *
 * paths_rank_joint: one rank per visited patch of a slide, jointly over the chosen levels.  scores [B, n_tot] fp32 (contiguous): the
 * capacities N_l of the L levels laid end to end; seg_end: DEVICE table [L] int32, seg_end[l] = N_0 + ... + N_l (ascending,
 * seg_end[L-1] <= n_tot; clamped by the kernel); level_on: DEVICE table [L] int32, non-zero = the level is chosen; num_ims [L, B]
 * int64.  Joint element j of level l (row r = j - seg_end[l-1]) is VALID iff level_on[l] != 0 and r < num_ims[l, b].  rank
 * [B, n_tot] int32: for a valid element the number of valid elements of the same slide that precede it in the total order (score
 * descending, joint index ascending; with ascending != 0 the score order is inverted, the index order is not), -1 otherwise; the
 * ranks of a slide's valid elements are a permutation of 0 .. count[b] - 1.  count [B] int32: the number of valid elements.
 * -0 orders as +0, +-inf are ordinary values, so the order is that of a stable descending (ascending) sort of the values; a NaN gets
 * some rank (the caller excludes them).  Scores of elements that are not valid are never read.  Rank counting on the 64-bit key of
 * paths_topk streamed through LDS in tiles of paths_rank_joint_tile() keys: n_tot is not bounded by LDS (1 <= n_tot <= 2^30,
 * L <= 16, B <= 65535).  No atomics, no workspace; the result does not depend on the launch geometry.
 *
 * paths_path_mask_points: the rows of C chunk members for B slides at one level, in the layout of paths_path_points (virtual slide
 * v = c * B + b; x [B, rows_per_slide, D] fp32 with element stride ldx between rows, a multiple of 4, >= D, 16-byte aligned base;
 * D % 128 == 0; base [D] fp32, 16-byte aligned, or NULL; out [C * B, rows_per_slide, D] contiguous, 16-byte aligned).  rank: this
 * level's slice of the joint rank, rank[b * ldr + r] (ldr >= rows_per_slide); thr [C, B] int32 and insert [C] int32: DEVICE tables;
 * num_ims [B].  For r < num_ims[b] the row is KEPT iff
 *     rank < 0                                   (the level is not perturbed), or
 *     insert[c] == 0 and rank >= thr[c, b]       (deletion: the first thr ranks are removed), or
 *     insert[c] != 0 and rank <  thr[c, b]       (insertion: only the first thr ranks are present);
 * a kept row is x[b, r, :] bit for bit, a removed row is base bit for bit (exact +0 when NULL).  Rows at or beyond num_ims[b] are not
 * read and get exact zeros.  One wavefront per recorded row, no arithmetic on the values, no workspace, no atomics. */
int paths_rank_joint_tile(void);
int paths_rank_joint(const float* scores, const int* seg_end, const int* level_on, const int64_t* num_ims, int L, int B, int n_tot,
                     int ascending, int* rank, int* count, paths_stream_t stream);
int paths_path_mask_points(const float* x, int64_t ldx, const float* base, const int* rank, int64_t ldr, const int* thr, const int* insert,
                           const int64_t* num_ims, int rows_per_slide, int D, int B, int C, float* out, paths_stream_t stream);

/* Removal curves on the free path (paths_amd/saliency.py:removal_curves; csrc/perturb_rows.hip): a member of a curve is a
 * slide with other tissue masks (DeviceSlide.with_masks), so the two kernels work on uint8 cell masks, one launch per level.
 *
 * paths_removal_masks: the masks of C members of B slides at one level.  src_ptrs: DEVICE table [B] of the addresses of the slides'
 * source masks (uint8 [gx[b], gy[b]], row-major; NULL table: every source is all zero); gx / gy: DEVICE tables [B] int32 of the
 * level's grid dims, max_cells >= every gx[b] * gy[b] (it sizes the launch); locs [B, N, 2] int64: the recorded locations in pixels,
 * cell = locs / patch_size, linear index cx * gy[b] + cy; num_ims [B] int64; rank: this level's slice of the joint rank,
 * rank[b * ldr + r] (ldr >= N); thr [C, B] int32 DEVICE table.  Row r of slide b is CHOSEN by member c iff r < num_ims[b] and
 * 0 <= rank < thr[c, b] (rank and thr both NULL: every valid row).  masks [C, B, ldm] uint8 (ldm >= max_cells, a multiple of 16,
 * 16-byte aligned base): bytes 0 .. gx[b] gy[b] - 1 of member (c, b) are the source mask with the cells of its chosen rows set to 0
 * (set != 0: to 1); the rest of the stride is not written.  left [C, B] int32: the non-zero bytes of that result.  The locations of
 * rows that are not chosen are never read (nor the ranks at or beyond num_ims[b]); a chosen location outside the grid is ignored.
 * Two valid rows of a slide never share a cell (the caller's contract): left is an integer count reduced in a fixed order, every
 * byte is written once - no atomics, no workspace, bit-identical on repeat.  16-byte copies where the source is 16-byte aligned.
 *
 * paths_visited_overlap: overlap[v] (int32 [C * B], v = c * B + b) = the number of rows r < num_m[v] of locs_m [C * B, Nm, 2] whose
 * cell is non-zero in bitmap[b * ldb + cell] (uint8; the cells the recorded pass of slide b visited at this level: a
 * paths_removal_masks result with set != 0 over a NULL source).  Integer count, fixed order, no atomics, no workspace.
 *
 * paths_level0_mask_rows: behind paths_level0_batch for a batch of masked views.  The reference loads every level-0 cell, background
 * included (an all-zero row); so for every level-0 cell j < gx[b] gy[b] whose mask byte (mask_ptrs: DEVICE table [B]) is 0 the copy
 * fts[b, j, :] (NULL: none) is zeroed and row_ptrs[b, j] (NULL: none) is pointed at zero_row.  Other rows are not touched. */
int paths_removal_masks(const int64_t* src_ptrs, const int* gx, const int* gy, int64_t max_cells, const int64_t* locs, int patch_size,
                        const int64_t* num_ims, const int* rank, int64_t ldr, const int* thr, int N, int B, int C, int set, uint8_t* masks,
                        int64_t ldm, int* left, paths_stream_t stream);
int paths_visited_overlap(const uint8_t* bitmap, int64_t ldb, const int* gx, const int* gy, const int64_t* locs_m, const int64_t* num_m,
                          int patch_size, int Nm, int B, int C, int* overlap, paths_stream_t stream);
int paths_level0_mask_rows(const int64_t* mask_ptrs, const int* gx, const int* gy, int B, int D, int64_t n0, float* fts, int64_t* row_ptrs,
                           const float* zero_row, paths_stream_t stream);

/* Heat-map rasters on the device, a whole batch per call (paths_amd/heatmap.py:rasterize; csrc/raster.hip; the data of
 * reference heatmap_visualise.py:147-171).  A raster is in finest cells: with L levels, f = 2^(L-1), slide b covers
 * [gx[b] f, gy[b] f] cells of the batch's padded [GX f, GY f] (gx / gy: DEVICE tables [B] int32 of the LEVEL-0 grids, clamped to
 * [0, GX] / [0, GY] by the kernels; GX / GY: the batch maxima); the patch of level l that covers finest cell (x, y) sits at cell
 * (x >> (L-1-l), y >> (L-1-l)) of that level's grid [GX << l, GY << l].
 *
 * paths_raster_index: the map from cell to visited row of ONE level.  locs [B, N, 2] int64 in pixels (cell = locs / patch_size),
 * num_ims [B] int64 (clamped to [0, N]).  index: int32 [B, GX << level, ldi] (ldi >= GY << level), every element -1 on entry
 * (written by the caller, pad columns included).  For every row i < num_ims[b] whose cell lies inside slide b's own grid
 * (gx[b] << level, gy[b] << level): index[b, cx, cy] = max(index[b, cx, cy], i) (integer atomicMax: of two rows on one cell the
 * later one stays, whatever the schedule).  A valid row with a negative location or a cell outside its slide's grid is skipped and
 * sets bit `level` of *status (int32, zeroed by the caller).  Rows of padding of locs (i >= num_ims[b]): never read.
 *
 * paths_raster_maps: all levels and slides in one launch, one thread per four consecutive finest cells of a raster row.
 * table: DEVICE table [L][4] int64 = (address of level l's index grid, its row stride ldi_l, address of level l's value rows,
 * their slide stride in elements): the value of row i of slide b is values_l[b * stride_l + i], fp32 (value_f64 = 0) or fp64 (1).
 * offset_w: DEVICE [2] fp64 = (offset, w).  With idx = index_l[b, x >> (L-1-l), y >> (L-1-l)]:
 *     v_l = idx >= 0 ? (double)(values_l[b, idx] + offset) : 0      the sum rounded in the VALUE's type (fp32 values: an fp32 add of
 *                                                                   the fp32-rounded offset, what NumPy computes for float32 + float)
 *     fold = 0 (planes):  out[b, l, x, y] = v_l                     out: [B, L, GX f, ldo]
 *     fold = 1:           for l = L-2 .. 0: v_l += w * v_{l+1} wherever the folded v_{l+1} != 0;  out[b, x, y] = v_0     out: [B, GX f, ldo]
 * in fp64, multiply and add rounded separately (no FMA); rounded once to the output type on the store: fp32 (out_f64 = 0) or fp64.
 * ldo >= GY f, a multiple of 4; out 16-byte aligned: every store is 16 bytes, columns [GY f, ldo) and all cells outside a slide's
 * own extent are written as +0.  Only rows an index grid names are read from the value rows (rows of padding: never read).  No
 * atomics, no LDS, a launch shape fixed by (B, GX, ldo, L): bit-identical on repeat.  1 <= L <= 8, B <= 65535. */
int paths_raster_index(const int64_t* locs, const int64_t* num_ims, const int* gx, const int* gy, int level, int patch_size, int N, int B,
                       int GX, int GY, int* index, int64_t ldi, int* status, paths_stream_t stream);
int paths_raster_maps(const int64_t* table, const int* gx, const int* gy, int L, int B, int GX, int GY, int value_f64, int out_f64, int fold,
                      const double* offset_w, void* out, int64_t ldo, paths_stream_t stream);

/* Overlays: a raster of the two entries above as 8-bit RGB pixels (paths_amd/heatmap.py:render; csrc/raster.hip; the
 * drawing of reference heatmap_visualise.py:148-181).  table, gx, gy, L, B, GX, GY as paths_raster_maps (the value columns of table are
 * not read); raster: the allocation paths_raster_maps wrote, fp32 (raster_f64 = 0) or fp64, row stride ldo; level = -1: its fold form
 * [B, GX f, ldo], level = l: plane l of its planes form [B, L, GX f, ldo].  The DRAWN levels are all levels for level = -1, else
 * level l alone.  A finest cell is VISITED when an index grid of a drawn level names a row on the cell that covers it and the
 * raster's value there is finite; the raster is read on cells an index grid of a drawn level names, and nowhere else.
 *
 * paths_render_range: range [B][2] fp64 = (vmin, vmax) per slide over its visited cells.  center = NULL: (min + 0.0, max + 0.0) of
 * the value (a -0 extreme becomes +0); center: DEVICE [1] fp64 z: m = max |value - z|, (z - m, z + m).  (0, 0) for a slide without a
 * visited cell.  status [B] int32: 1 when a cell a drawn index grid names holds a non-finite value, else 0.  Two launches of fixed
 * shape (64 partial blocks per slide, then one thread per slide), no atomics: min / max of finite values do not depend on the
 * order, so the result is bit-identical on repeat.  partial: workspace of B * 64 * 3 fp64.
 *
 * paths_render_rgb: out uint8 [B, GX f c, ldp], c = cell_px in [1, 64], ldp a multiple of 16 and at least GY f c * 3 bytes, out
 * 16-byte aligned; pixel (u, v) of slide b at bytes [3 v, 3 v + 3) of row u shows finest cell (u / c, v / c).  All slides in one
 * launch, one thread per 16 consecutive pixels of a row (three 16-byte stores).  With (vmin, vmax) = range[b], in fp64 with every
 * operation rounded separately:
 *     t256 = (value - vmin) / (vmax - vmin) * 256.0;  k = t256 >= 255 ? 255 : t256 > 0 ? (int)t256 : 0;  k = 0 when vmax == vmin
 *     visited pixel:  (alpha255 * colours[k] + (255 - alpha255) * under + 127) / 255 per channel, in integers
 *     other pixels of the slide's extent:  under
 * colours: DEVICE [256] uint32 = r | g << 8 | b << 16; under = background (same packing), or with thumbs != NULL the pixel of the
 * slide's thumbnail: thumbs DEVICE [B][2] int64 = (address of a uint8 image [gx[b] f c, gy[b] f c, 3] with pixel stride 3, its row
 * stride in bytes).  Outlines, painted last and opaque, whatever the value: for every level l of the bit mask outline_levels whose index
 * grid names a row on the cell covering a pixel, the pixel takes outline_rgb when it lies in the first or last pixel row or column of
 * that cell (which spans c << (L-1-l) pixels).  Pixels outside a slide's own extent and the pad bytes of every row are written as 0:
 * every byte of out is written, none is read.  No atomics, no LDS: bit-identical on repeat. */
int paths_render_range(const int64_t* table, const int* gx, const int* gy, int L, int B, int GX, int GY, int level, const void* raster,
                       int raster_f64, int64_t ldo, const double* center, double* partial, double* range, int* status, paths_stream_t stream);
int paths_render_rgb(const int64_t* table, const int* gx, const int* gy, int L, int B, int GX, int GY, int level, const void* raster,
                     int raster_f64, int64_t ldo, const double* range, const uint32_t* colours, const int64_t* thumbs, int cell_px, int alpha255,
                     int outline_levels, uint32_t outline_rgb, uint32_t background, uint8_t* out, int64_t ldp, paths_stream_t stream);

/* Annotation polygons (paths_amd/annotations.py; csrc/polygons.hip; the polygons reference heatmap_visualise.py:21-48,
 * 123-135 draws beside the heat map).  The NumPy statement of both entries is tests/polygon_ref.py; the kernels equal it bit for bit.
 *
 * FIXED POINT.  A coordinate is an int32 with 16 fractional bits per FINEST cell (one cell of a raster above = 65536), (row, col) with
 * row along the grid's X.  verts int32 [V][2]; polygon k owns vertices poly_off[k] .. poly_off[k+1] - 1 (poly_off int32 [P + 1],
 * ascending, at least 3 each) and is closed implicitly: its edges run a -> b from each vertex to the next and from the last to the
 * first; slide b owns polygons slide_poly[b] .. slide_poly[b+1] - 1 (int32 [B + 1]).  The kernels clamp every offset into its array,
 * so no table can make them read outside verts.  gx / gy: DEVICE [B] int32, the slide's own extent in FINEST cells, clamped to [0, X] /
 * [0, Y].  Bounds the host keeps (annotations.Polygons refuses, never clamps): |coordinate| <= 2^29, extents <= 8192 cells = 2^29,
 * V <= 2^20.  A sample point lies in [0, 2^29), so every difference of two coordinates is at most 2^30 in magnitude, each of the
 * two products of t below at most 2^60 and t itself below 2^61: exact in int64.
 *
 * paths_polygon_cover: out int32 [B, X, ld] (ld >= Y); out[b, x, y] = the number of the s x s sample points of finest cell (x, y),
 * s = samples in {1, 2, 4, 8, 16}, that lie inside the union of slide b's polygons; sample (i, j) is the point
 * p = ((x << 16) + o_i, (y << 16) + o_j), o_i = ((2 i + 1) << 15) >> log2 s.  Polygon k contains p by the even-odd rule: the parity
 * of its edges a -> b with (a.r > p.r) != (b.r > p.r) whose crossing lies beyond p.c, i.e. with d = b.r - a.r and
 * t = (p.c - a.c) * d - (p.r - a.r) * (b.c - a.c) in int64: t < 0 when d > 0, t > 0 when d < 0.  A sample is inside when any polygon
 * contains it (holes by parity within a polygon, none between polygons).  Cells outside the slide's own extent and columns [Y, ld)
 * are written as 0: every element of out is written, none is read.  One launch for the batch: a workgroup owns 16 x 16 cells and
 * streams the slide's edges, polygon by polygon, through one LDS tile of 256 edges, keeping an edge only when its row span meets the
 * tile's sample rows and it does not lie wholly on the near side of the tile's sample columns (where no crossing can lie beyond p.c);
 * an edge wholly beyond a cell's sample columns costs that cell the row test alone.  No atomics, no workspace; parity and union are
 * order-free, so the result is bit-identical on repeat.  B <= 65535, X, Y <= 8192.
 *
 * paths_polygon_outline: draws every edge in place on uint8 RGB images, images DEVICE [B][2] int64 = (address of slide b's image
 * [gx[b] c, gy[b] c, 3] with pixel stride 3, its row stride in bytes), c = cell_px in [1, 64].  An endpoint's pixel is
 * floor(coordinate * c / 65536) per axis.  With (du, dv) the difference of the endpoint pixels and n = max(|du|, |dv|), the edge
 * paints k = 0 .. n at (u0 + floor((2 k du + n) / (2 n)), v0 + floor((2 k dv + n) / (2 n))), for n = 0 the pixel (u0, v0) alone.  A
 * painted pixel (u, v) is the square [u - width / 2, u - width / 2 + width) x [v - width / 2, ...) (integer division; width in
 * [1, 7]), clipped to the slide's own extent, every byte triple of it = rgb (r | g << 8 | b << 16), opaque.  cum: DEVICE int32
 * [V + 1], cum[e] = the sum of n + 1 over the edges before edge e (edge e starts at vertex e), steps = cum[V] < 2^31 - 256: one
 * thread per (edge, step), one launch for the batch.  Every writer of a byte writes the same value, so the order of the writers
 * cannot matter and the image is bit-identical on repeat; plain byte stores, no atomics.  Bytes no edge paints are neither read nor
 * written. */
int paths_polygon_cover(const int* verts, int V, const int* poly_off, int P, const int* slide_poly, const int* gx, const int* gy, int B, int X,
                        int Y, int samples, int* out, int64_t ld, paths_stream_t stream);
int paths_polygon_outline(const int* verts, int V, const int* poly_off, int P, const int* slide_poly, const int* gx, const int* gy, int B,
                          const int* cum, int64_t steps, const int64_t* images, int cell_px, int width, uint32_t rgb, paths_stream_t stream);

/* z = alpha * x (+ h on valid rows): importance scaling and the non-LSTM hierarchical-context add
 * (reference model/paths.py:96-109). */
int paths_scale_add_rows(const float* x, const float* alpha, const float* h, const int64_t* num_ims, int rows_per_slide,
                         int D, int64_t M, int use_alpha, float* z, paths_stream_t stream);

/* Tissue mask of a preprocessed grid [cells, D]: 1 iff fp32 row sum != 0 (reference slide.py:324). */
int paths_tissue_mask(const float* grid, int64_t cells, int D, uint8_t* mask, paths_stream_t stream);

/* The same pass (mask may be NULL) + *absmax_bits = max(*absmax_bits, fp32 bit pattern of max|x| over the grid): non-negative
 * floats order like their bit patterns, a NaN reads back above +inf.  Guards the fp16-split range contract of the default mode
 * (replaces nothing in the reference; its fp32 CPU path has no such limit). */
int paths_tissue_mask_absmax(const float* grid, int64_t cells, int D, uint8_t* mask, uint32_t* absmax_bits, paths_stream_t stream);
/* paths_tissue_mask_absmax over an FP16 grid [cells, D] (sums and max|x| in fp32: the same mask and bits as the fp32 grid of the same values). */
int paths_tissue_mask_absmax_h16(const void* grid, int64_t cells, int D, uint8_t* mask, uint32_t* absmax_bits, paths_stream_t stream);

/* Counter-based synthetic grid (paths_amd/synthetic.py). */
int paths_synth_grid(float* grid, int X, int Y, int D, uint32_t slide_level_key, int level, uint64_t bg_threshold,
                     paths_stream_t stream);
/* paths_synth_grid into an FP16 grid: the same values rounded to nearest even. */
int paths_synth_grid_h16(void* grid, int X, int Y, int D, uint32_t slide_level_key, int level, uint64_t bg_threshold,
                         paths_stream_t stream);

/* lstm = false training (reference model/paths.py:95-109, Z = alpha X + hctx): gradient of the importance MLP through the row
 * scaling: dalpha = dZ . X per row, dz = valid dalpha alpha (1 - alpha); dh [M,128] = (hid > 0) dz w2, dah = dz hid, da = dz. */
int paths_importance_rows_bwd(const float* dz_rows, const float* x, int D, const float* hid, const float* alpha, const float* w2,
                              const int64_t* num_ims, int rows_per_slide, int64_t M, float* dh, float* da, float* dah,
                              paths_stream_t stream);

/* ---- dropout (training; reference nn.Transformer(..., dropout=p), model/aggregator.py:25-33: attention probabilities,
 * dropout1, dropout2, the feed-forward's inner dropout, dropout3).  Masks are never stored: element idx of site `key` is kept iff
 * the 16-bit half (low for even idx, high for odd) of hash(idx & ~1, key) is >= round(p * 65536) (csrc/dropout.h: one 32-bit hash
 * per pair of elements) and is regenerated by every kernel that needs it; kept values are scaled by 1 / (1 - p16), p16 =
 * round(p * 65536) / 65536 the rate actually applied.  Attention probabilities of (slide, head) pair s: element (query q, key k)
 * has idx = (s * T + q) * T' + k with T' = T rounded up to even.  The host derives one 64-bit key per (step seed, level, layer, site). */

/* out[r, c] = (resid ? resid[r, c] : 0) + (vec ? vec[c] : x[r, c]) * mask(r * N + c) / (1 - p16); exactly one of x / vec is given;
 * x, resid, out may alias.  Covers dropout1 / dropout3 (+ residual), the inner feed-forward dropout (in place), dropout2 on the
 * broadcast cross-attention bias (vec) and the masking of gradients in the backward pass. */
int paths_dropout_rows(const float* x, int64_t ldx, const float* vec, const float* resid, int64_t ldr, float* out, int64_t ldo,
                       int64_t M, int N, uint64_t key, float p, paths_stream_t stream);
/* mask[i] = 1 kept / 0 dropped, i in [0, n): tests only */
int paths_dropout_mask(float* mask, int64_t n, uint64_t key, float p, paths_stream_t stream);
/* Opt-in low-precision variant for the stress geometry (BASELINE.json configs[4]): the same attention with OCP e4m3 operands, one
 * v_mfma_f32_16x16x32_fp8_fp8 per product block (csrc/attn_fp8.hip).  4 significant bits per operand: NOT within the 1e-4 logit bar;
 * never used unless PATHS_ATTN_FP8=1.  workspace: paths_attention_fp8_workspace(B, T, H, head_dim) bytes. */
int64_t paths_attention_fp8_workspace(int B, int T, int H, int head_dim);
int paths_attention_fp8(const float* q, const float* k, const float* v, float* o, const int64_t* num_ims, int B, int T, int H,
                        int head_dim, void* workspace, paths_stream_t stream);
/* The same on the token-major in_proj output qkv [B*T, 3d] (row stride ld; q unscaled, qscale = log2(e)/sqrt(head_dim) applied while the
 * operand images are written); head_dim 32 or 64. */
int paths_attention_fp8_qkv(const float* qkv, int64_t ld, float* o, const int64_t* num_ims, int B, int T, int H, int head_dim, float qscale,
                            void* workspace, paths_stream_t stream);

/* e4m3 GEMM of the stress variant (csrc/gemm_fp8.hip: v_mfma_scale_f32_32x32x64_f8f6f4, unit block scales, per-tensor scales) for the
 * aggregator's products over all tokens (reference model/aggregator.py:25-33: in_proj, out_proj, linear1, linear2).  Opt-in, NOT a parity
 * path (4 significant bits per operand).
 *   paths_fp8_scale        *scale = 448 / max|x| over an fp32 [M, K] matrix, on the device (scratch: one zeroed uint32, left zero);
 *                          with num_ims / rows_per_slide only the valid token rows of a token-major activation count
 *   paths_fp8_pack_weight  w8 [ceil(N/256)*256, K] = e4m3(W * *scale) (zero rows behind N), *scale = 448 / max|W|; K % 64 == 0
 *   paths_fp8_quantize     x8 [ceil(M/256)*256, K] = e4m3(x * *scale) of an fp32 [M, K] matrix (zero rows behind M)
 *   paths_gemm_nt_fp8      out[M,N] = act(A W^T + bias) (+ residual) from the two e4m3 images and their scales; K % 128 == 0 */
int paths_fp8_scale(const float* x, int64_t ld, int64_t M, int K, float* scale, unsigned int* scratch, const int64_t* num_ims,
                    int rows_per_slide, paths_stream_t stream);
int paths_fp8_pack_weight(const float* w, int64_t ldw, int N, int K, uint8_t* w8, float* scale, unsigned int* scratch, paths_stream_t stream);
int paths_fp8_quantize(const float* x, int64_t ld, int M, int K, const float* scale, uint8_t* x8, paths_stream_t stream);
int paths_gemm_nt_fp8(const uint8_t* a8, const uint8_t* w8, const float* a_scale, const float* w_scale, const float* bias,
                      float* out, int64_t ldo, int M, int N, int K, int act, const float* residual, int64_t ldr, paths_stream_t stream);
/* The same product handed on in e4m3 (the A image of the next GEMM): out8 [ceil(M/256)*256, N] = e4m3(act(A W^T + bias) * *out_scale),
 * rows >= M zero on entry; *out_scale is a calibrated per-tensor scale, out_absmax (optional) receives max|result| as float bits. */
int paths_gemm_nt_fp8_out8(const uint8_t* a8, const uint8_t* w8, const float* a_scale, const float* w_scale, const float* bias,
                           uint8_t* out8, const float* out_scale, unsigned int* out_absmax, int M, int N, int K, int act,
                           paths_stream_t stream);

/* paths_attention_x6 with dropout on the softmax probabilities: O = (softmax(S) * mask / (1 - p)) V, lse un-dropped; mask element
 * ((b * H + h) * T + q) * T + k.  q, k, v fp32 (no pre-built images). */
int paths_attention_x6_dropout(const float* q, const float* k, const float* v, float* o, float* lse, const int64_t* num_ims, int B,
                               int T, int H, int head_dim, int max_queries, void* workspace, int planes, uint64_t drop_key,
                               float drop_p, paths_stream_t stream);
/* backward twins (same key, same p as the forward) */
int paths_attention_bwd_f32_dropout(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                                    const float* lse, const int64_t* num_ims, float* dqkv, float* ws_dsum, int B, int T, int H,
                                    int head_dim, uint64_t drop_key, float drop_p, paths_stream_t stream);
/* The same with the dQ part on the split-bf16 matrix-core kernel (csrc/attn_bwd_x6.hip: three exact bf16 planes per operand, as
 * accurate as the f32 MFMA); images: paths_attention_bwd_x6_workspace(B, T, H, head_dim) bytes of scratch. */
int64_t paths_attention_bwd_x6_workspace(int B, int T, int H, int head_dim);
int paths_attention_bwd_x6_dropout(const float* q, const float* k, const float* v, const float* o, const float* d_o, const float* lse,
                                   const int64_t* num_ims, float* dqkv, float* ws_dsum, void* images, int B, int T, int H, int head_dim,
                                   uint64_t drop_key, float drop_p, paths_stream_t stream);
/* The same with the operand split chosen by the caller: planes 3 = three exact bf16 planes (6 MFMAs per product block), planes 2 =
 * hi | mid only (16 significant bits at fp32's exponent range, 3 MFMAs: what the training step's gradient GEMMs use by default). */
int paths_attention_bwd_x6_planes(const float* q, const float* k, const float* v, const float* o, const float* d_o, const float* lse,
                                  const int64_t* num_ims, float* dqkv, float* ws_dsum, void* images, int B, int T, int H, int head_dim,
                                  uint64_t drop_key, float drop_p, int planes, paths_stream_t stream);

/* ---- wide heads (head_dim > 64, a multiple of 32: e.g. trans_dim 256 / 2 heads, or 1536 / 4 heads = 384, the stress form of
 * BASELINE configs[4]; reference model/aggregator.py:25-33 accepts any trans_dim % trans_heads == 0).  Per (slide, head): S = q k^T
 * (f32-input MFMA GEMM), masked softmax, O = P V, and the corresponding five products backward, with the score matrix in scratch
 * (paths_attention_wide_workspace floats).  Same conventions as paths_attention_any_train / paths_attention_bwd_any; qkv must have at
 * least 128 readable rows behind its last one. */
int64_t paths_attention_wide_workspace(int T, int head_dim);
int paths_attention_wide_fwd(const float* qkv, int64_t ld, float* o, float* lse, const int64_t* num_ims, int B, int T, int H, int head_dim,
                             float qscale, int max_queries, uint64_t drop_key, float drop_p, float* workspace, paths_stream_t stream);
int paths_attention_wide_bwd(const float* qkv, int64_t ld, const float* o, const float* d_o, const float* lse, const int64_t* num_ims,
                             float* dqkv, int B, int T, int H, int head_dim, float qscale, int max_queries, uint64_t drop_key, float drop_p,
                             float* workspace, paths_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PATHS_HIP_H */
