/* coponerf_hip.h — C ABI of libcoponerf_hip.so (gfx950 / MI355X).
 *
 * The upstream reference (cvlab-kaist/CoPoNeRF) has no FFI: its hot path is a
 * chain of ATen calls inside models/CoPoNeRF.py:208-576.  Each entry point
 * below replaces one group of those calls; the Python class
 * coponerf_amd.CoPoNeRF.CoPoNeRF (same constructor / get_z / forward contract
 * as models/CoPoNeRF.py:19-576) binds them through ctypes (coponerf_amd/_hip.py).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named host_*; nothing is
 *     allocated or freed by the library; outputs are caller-allocated.
 *   - return value: 0 = ok, otherwise a negative argument error (CPN_E_*) or a
 *     positive hipError_t; cpn_last_error() gives a message.  Never throws.
 *   - `stream` is a hipStream_t passed as void* (the caller's current stream).
 *   - fp16 buffers are IEEE binary16 ("half"), declared as uint16_t here.
 *   - N = B*V camera slots, ordered n = b*V + v  (V == 2).
 *   - "sample arrays" are (N,R,S,·) ; "row arrays" feed the GEMMs and are ordered
 *       row = (((b*R + r)*V + v)*S + s)*J + j        J = 2 encoder inputs per sample
 *     so that all V*S*J rows of one query ray are contiguous.
 */
#ifndef COPONERF_HIP_H
#define COPONERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPN_ABI_VERSION 12   /* cpn_attend_units (round 7), cpn_ssim_warp* (round 8), cpn_image_metrics* (round 9), summaries.hip (round 10), lpips.hip (round 11), novel_views.hip (round 12), epipolar.hip (round 13), cpn_lpips_*_bwd (round 14), point_cloud.hip (round 15), matches.hip (round 16), splat.hip (round 17), mesh.hip (round 18), raster.hip (round 19), ransac.hip (round 20), ransac5.hip (round 21) and ransac_h.hip (round 22) are additive - symbols added, none altered: the version stays */

#define CPN_E_ARG   (-1)   /* bad argument (null pointer, size, alignment) */
#define CPN_E_SHAPE (-2)   /* shape not supported by the compiled tiles    */

/* camera block: CPN_CAM_STRIDE floats per (b,v), built on the host from 4x4 matrices */
#define CPN_CAM_STRIDE 96
#define CPN_CAM_TQ    0    /* 16: query camera -> frame of context view v   (CoPoNeRF.py:241-244) */
#define CPN_CAM_M     16   /* 16: inv(c2w_v) @ c2w_v, ~identity             (CoPoNeRF.py:239)     */
#define CPN_CAM_AOWN  32   /* 16: view-v frame -> view-v frame              (CoPoNeRF.py:326-332) */
#define CPN_CAM_AOTH  48   /* 16: view-v frame -> frame of the other view                          */
#define CPN_CAM_KQ    64   /* fx fy cx cy of the query camera, pixel units                         */
#define CPN_CAM_KC    68   /* fx fy cx cy of context view v                                        */
#define CPN_CAM_KO    72   /* fx fy cx cy of the other context view                                */
#define CPN_CAM_KN    76   /* 9: K_v[:3,:3] with rows 0,1 divided by H      (CoPoNeRF.py:259-261) */

/* padded K of the first encoder layer: 835 inputs -> 864 consumed (27 x 32); row stride 896 halves = 14 x 128 B:
 * 128-byte-aligned rows are worth 10 % on the GEMM that reads them (808 vs 728 TFLOP/s, measured in round 1 with a leading-dimension sweep of tools/gemm_bench.py) */

int         cpn_abi_version(void);
const char* cpn_last_error(void);

/* ---- CU-partitioned streams -------------------------------------------------------------------------------------
 * The reference's evaluation loop runs get_z and the chunked forward() calls strictly one after the other
 * (test.py:164-212, wrapper.py:176-211).  On an MI355X the render pass (HBM-bound, persistent grids on every CU) and
 * get_z (hundreds of small launches) only overlap when each has CUs of its own: a stream created here is restricted
 * to CUs [first_cu, first_cu + num_cus) of the CU-mask order, which KFD spreads round-robin over the 8 XCDs and their
 * 4 shader engines — both numbers must be multiples of 32, i.e. an equal share of every shader engine of every XCD.  The persistent launchers of this library
 * (cpn_encode_key, cpn_gemm_f16*) size their grids by cpn_stream_cu_count(stream).  `stream_out` receives a
 * hipStream_t; destroy it with cpn_stream_destroy once its work has completed.  (coponerf_amd/streams.py, pipeline.py) */
int cpn_device_cu_count(void);
int cpn_stream_cu_count(void* stream);
int cpn_stream_create_cu_range(int first_cu, int num_cus, void** stream_out);
int cpn_stream_destroy(void* stream);

/* ---- K1: query rays -> Pluecker coords + clipped epipolar segment ------------------------------
 * replaces geometry.plucker_embedding (utils_training/geometry.py:236-245, :426-433, :409-419, :353-371),
 * epipolar.project_rays (models/epipolar.py:175-253) and the start/end scrub (models/CoPoNeRF.py:279-291).
 *   cam     (N, CPN_CAM_STRIDE)        uv: pixel (x = column, y = row) of ray r of pair b at uv[b*uv_batch_stride + 2r]
 *                                      (2R for a dense (B,R,2) array; a ray chunk of a larger array passes its stride)
 *   coords9 (N,R,9)  = dir3 | moment3 | origin3
 *   seg     (N,R,4)  = start.xy | end.xy in [-1,1], NaN/Inf -> 0
 *   overlaps(N,R)    uint8 0/1                                                                   */
int cpn_project_rays(const float* cam, const float* uv, long long uv_batch_stride, int B, int V, int R,
                     float* coords9, float* seg, uint8_t* overlaps, void* stream);

/* ---- K1b: per-sample geometry -------------------------------------------------------------------
 * replaces sample generation (CoPoNeRF.py:294-309), geometry.get_3d_point_epipolar / get_intersection
 * (geometry.py:98-162, float64 inside), utils.encode_relative_point (utils.py:99-108), geometry.project +
 * utils.normalize_for_grid_sample (geometry.py:374-393, utils.py:242-245), geometry.get_ray_directions_cam
 * (geometry.py:313-324) and the depth encoding (CoPoNeRF.py:428-445).
 *   interval (S) = linspace(0,1,S) as the host computes it
 *   pixel_val (N,R,S,2)   pt (N,R,S,3)   sec_grid (N,R,S,2): coords of this sample's 3-D point in the OTHER image
 *   pe6 (N,R,S,6) = tanh(nan_to_num(pt_own)/5) | tanh(nan_to_num(pt_other)/5)
 *   loc8 (N,R,S,8) = context-pixel ray dir 3 | tanh(depth*{1,.1,.01,.001}) 4 | 0
 *   lv_u, optional (NULL: not written): (B * ceil(R/4) * V * ceil(S/4) units, 64 lanes, 4) fp32 - the 16 local_coords inputs of
 *       every sample (loc8's 7 values, 6 of coords9, a 1.0 for the bias, zeros; CoPoNeRF.py:411-445) in the UNIT order of
 *       cpn_local_units: lane c + 16 fg of unit ((b * ceil(R/4) + r/4) * V + v) * ceil(S/4) + s/4, c = (s & 3) * 4 + (r & 3),
 *       holds K entries 4 fg .. 4 fg + 3 = {dir3, 1} | {0, 0, c9[0], c9[1]} | {c9[2], tanh(depth * {1, .1, .01})} |
 *       {tanh(depth / 1000), c9[6..8]}.  Slots of rays >= R / samples >= S are written as zeros.                               */
int cpn_sample_geometry(const float* cam, const float* coords9, const float* seg, const float* interval,
                        int B, int V, int R, int S, int H, int W,
                        float* pixel_val, float* pt, float* sec_grid, float* pe6, float* loc8, float* lv_u, void* stream);

/* ---- layout: (N,C,h,w) fp32 -> (N,h,w,C) fp16 feature map (once per get_z) --------------------- */
int cpn_nchw_to_nhwc_f16(const float* src, uint16_t* dst, int N, int C, int h, int w, void* stream);

/* ---- pack a (N_out, K_in) fp32 weight into fp16 [N_out][ld] with zero padding (once per weight version) */
int cpn_pack_weight_f16(const float* src, int n_out, int k_in, uint16_t* dst, int ld, void* stream);

/* ---- small fp32 first layers feeding the attention MLPs --------------------------------------------
 * out[row, 0:128] = fp16( relu( W[:, 0:16] . L(row) + bias + add[ray, 0:128] ) ),  rows = (b,r,v,s), ray = (b,r)
 * with L = [loc8 dir 3 | 0 0 0 | query dir 3 | loc8 depth 4 | query origin 3]      (CoPoNeRF.py:445)
 * query_embed (CoPoNeRF.py:446): w = query_embed.weight (128,16), add = NULL
 * query_repeat_embed (CoPoNeRF.py:472-473): w = weight[:, 128:144] (ld 144), add = weight[:, :128] . z_embed + 0 */
int cpn_local_hidden(const float* loc8, const float* coords9, const float* w, int ldw, const float* bias,
                     const float* add, int B, int V, int R, int S, int ray0, int nrays, uint16_t* out, void* stream);

/* ---- K2+K3a: first encoder layer straight from the feature maps ("project, then interpolate") -------------------
 * hid = ReLU(query_encode_latent([primary/secondary gather (832) | tanh(pt/5) (3)])) without the gathered rows ever
 * reaching HBM; replaces F.grid_sample x 8, torch.cat and the 835 -> 832 1x1 convolution (CoPoNeRF.py:312, 370,
 * 384-397 with the layer of :71).  A 1x1 convolution commutes with bilinear interpolation, and the texel centres of the
 * three 256-channel levels (H/16, H/8, H/4; align_corners=False) all lie on the nodes of one grid of spacing 2/W, on
 * whose cells every level's interpolant is bilinear — so the projected sum of the three levels is tabulated once per
 * stereo pair on that grid and interpolated from 4 nodes (exact in real arithmetic; csrc/encode.hip):
 *   per image  T_border (H/2+1, W/2+1, CPN_TAB_LD) fp16   nodes 0..M         own image, 'border' padding
 *              T_zeros  (H/2+9, W/2+9, CPN_TAB_LD) fp16   nodes -4..M+4      other image, 'zeros' padding
 *   laid out image by image, border table first: cpn_encode_table_nodes(H, W) nodes (rows) per image.
 *   Built as  cpn_node_features (the three levels sampled at every node -> (nodes, 768) fp16)
 *             -> cpn_gemm_f16(A = node features, W = wtab, N = CPN_TAB_LD, K = 768, bias 0, fp16 out).
 * A row is then 4 weighted table taps + a K = 80 MFMA product over [level-3 gather (64) | pt (3) | bias hi, lo | 0].
 * Table rows hold the 832 channels in natural order (1664 B, 13 cache lines; the kernel walks 13 slices of 64 channels).
 *   cpn_pack_encode_weights: W (832, ldw >= 835) fp32 query_encode_latent.weight ->
 *       wfrag (CPN_ENC_FRAG_HALVES halves) MFMA A-operand fragments of W[:, 768:835] (K padded to 96)
 *       wtab  (832, 768) fp16 table projection weights W[:, 0:768]
 *   the layer itself: cpn_encode_key below (until round 5 also as a kernel without the key layer, cpn_encode_hidden)  */
#define CPN_TAB_LD    832
#define CPN_NODE_PAD  4
#define CPN_ENC_FRAG_HALVES (13 * 3 * 4 * 64 * 8)
long long cpn_encode_table_nodes(int H, int W);
int cpn_pack_encode_weights(const float* W, int ldw, uint16_t* wfrag, uint16_t* wtab, void* stream);
int cpn_node_features(const uint16_t* map0, const uint16_t* map1, const uint16_t* map2, int H, int W, int nimg,
                      uint16_t* out, void* stream);
/* cpn_encode_key (csrc/encode_fused.hip; round 5 form of round 4's kernel): the first layer with the folded key_map layer
 * behind it (models/CoPoNeRF.py:404-407 after :387-397; folding: DESIGN.md 4.3) - the 64-channel slices of hid are the K panel
 * of the 1664 -> 128 contraction while they are still in registers, so the key path never reads hid back from HBM.
 *   kwring (2 images, 13 slices, 8 tiles, 2 k steps, 64 lanes = row + 16 * 8-column group, 8) fp16: the folded key matrix
 *       (Wk_a W2 | Wk_b W2) (128, 1664) in the order the kernel streams it through its two-slot LDS ring - piece (t, k) of slice
 *       step (j, n) holds, in lane (a, g), W'[16 t + a][832 j + 64 n + 32 k + 8 g .. +8]: every 1 KiB DMA piece is contiguous;
 *       kbias (128) fp32 = Wk_a b2 + Wk_b b2 + bk
 *   hid (rays*V*S*2, 832) fp16 in the row order of this header (written: the two hidden sums read it); bias (832) fp32; map3 the
 *       full-resolution NHWC fp16 map (N, H, W, 64); kh (rays*V*S, 128) fp16 = ReLU(W' . [hid_own ; hid_other] + kbias), rows in
 *       the order of this header; kh is bit-identical to cpn_gemm_f16(hid, W', relu).
 *   kh_units = 1: kh leaves in UNIT order instead of row-major - the 16 rows of a unit (4 adjacent rays x 4 consecutive samples of
 *       one view; unit u of a launch = ((ray group - first group) * V + view) * ceil(S/4) + sample block, cpn_encode_units() of them)
 *       as [unit][32-column block p][lane = c + 16 fg][8] = kh[row(unit, c)][32 p + 8 fg .. +8], c = (sample & 3) * 4 + (ray & 3):
 *       every store of a wave is 1 KiB of contiguous memory and every block is a ready MFMA B fragment for cpn_local_units.
 *       The buffer holds cpn_encode_units() * 16 rows (dead rows of partial units included).                                */
int cpn_encode_key(const uint16_t* tab, const uint16_t* map3, int H, int W, const float* pixel_val,
                   const float* sec_grid, const float* pe6, const uint16_t* wfrag, const float* bias,
                   const uint16_t* kwring, const float* kbias, int B, int V, int R, int S, int ray0, int nrays,
                   uint16_t* hid, uint16_t* kh, int kh_units, void* stream);
long long cpn_encode_units(int B, int R, int S, int ray0, int nrays);
/* ---- the per-sample query / key tails of the two attention rounds in UNIT order (round 5, csrc/local_units.hip) ------------
 * mode 0 (CoPoNeRF.py:408, 446, 450): ce = query_embed_2(ReLU(query_embed(local_coords))) -> ce_u (unit order, cpn_encode_units()
 *   * 16 rows); logits[row] = < fp16(key_map_2(kh_u[row])), fp16(ce[row]) >, kh_u = cpn_encode_key's unit-order output.
 *   w1 (128, ldw1 >= 16) fp32 / b1: first layer; w2 (128, ldw2) fp16 / b2: second layer;
 *   wk2 (128, ldwk2) fp16 / bk2: key_map_2.
 * mode 2 (:472-475): logits[row] = < fp16(query_repeat_embed_2(ReLU(w1 . local_coords + b1 + add[ray]))), ce[row] >, add (nrays,
 *   128) fp32, with coords_embed RECOMPUTED from the local coordinates (the same instructions in the same order as mode 0 formed
 *   it with).  logits (nrays*V*S) fp32 in row order; rows of a partial unit outside the ray range are skipped.  w1b (128, ldw1b >= 16) fp32 / b1b = query_embed, wk2 / bk2 =
 *   query_embed_2; ce_u is not touched.  Mode 0 with ce_u = NULL then stores no coords_embed at all (2 x 256 bytes per sample
 *   less HBM traffic; both kernels were bound by it).  w1b / b1b are ignored by mode 0.  (Mode 1 - round 2 reading a stored
 *   coords_embed - left the library in round 6.)
 *   lv_u, optional (NULL: the kernel reads loc8 / coords9 itself): the unit-order copy of the rows' 16 first-layer inputs that
 *   cpn_sample_geometry writes for the WHOLE (B, R, S) problem - every mode then reads ONE coalesced 1 KiB line per unit instead
 *   of five scattered 4 - 16 byte accesses per lane (the same values: the same logits); the launch's units start at its first
 *   ray group inside it.                                                                                                    */
int cpn_local_units(int mode, const float* loc8, const float* coords9, const float* w1, int ldw1, const float* b1,
                    const float* add, const uint16_t* w2, int ldw2, const float* b2, const uint16_t* wk2, int ldwk2,
                    const float* bk2, const float* w1b, int ldw1b, const float* b1b, const uint16_t* kh_u, int B, int V,
                    int R, int S, int ray0, int nrays, uint16_t* ce_u, const float* lv_u, float* logits, void* stream);

/* ---- K3: fused GEMM  C = act(A . W^T + bias), fp16 in, fp32 accumulate (MFMA 16x16x32 f16) -----------
 * replaces the per-sample 1x1 convolutions (CoPoNeRF.py:387-397, 404, 408, 446, 473).
 *   A (M, lda) fp16, W (N, ldw) fp16 (both K-contiguous), bias (N) fp32, K multiple of 32, N multiple of 16*tile
 *   out_f32 = 0: C fp16 (M, ldc) ; 1: C fp32 (M, ldc) ; 2: C fp32 += the product + bias, then the ReLU (round 6)        */
int cpn_gemm_f16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias,
                 void* C, int ldc, int M, int N, int K, int relu, int out_f32, void* stream);
/* Few-row form (round 4): the per-RAY value projection of a small call (M = 3 641 rays when the callers render an image as 18
 * forward() calls, test.py:176-190) - fp32 out, results bit-identical to cpn_gemm_f16 (same accumulation order), 13 us where
 * the 256-row tiles take 37.  Wp = the weights in MFMA fragment order, written once per parameter version by
 * cpn_pack_gemm_frags: (N/16, K/32, 64 lanes, 8) fp16, lane l of fragment (t, ks) = W[16 t + (l & 15)][32 ks + 8 (l >> 4) .. +8]. */
int cpn_pack_gemm_frags(const uint16_t* W, int ldw, int N, int K, uint16_t* out, void* stream);
int cpn_gemm_f16_fewrows(const uint16_t* A, int lda, const uint16_t* Wp, const float* bias, float* C, int ldc, int M, int N,
                         int K, int relu, void* stream);

/* ---- K4': the same joint softmax, reducing the 1664 hidden activations [h_own ; h_other] of every sample ----
 * (value projection folded through query_encode_latent_2 and applied once per ray afterwards)
 *   hid (rays*V*S, 1664) fp16 = the (rows*2, 832) output of the first encoder layer; hbar (rays, 1664) fp16   */
/*   logits (rays*V*S) fp32 or NULL: the row dot products <qa[row], qb[row]> when the producing kernel already
 *   formed them (cpn_local_units); then qa, qb may be NULL                                                     */
int cpn_attend_hidden(const uint16_t* qa, const uint16_t* qb, const float* logits, const uint16_t* hid, int B, int V,
                      int R, int S, int ray0, int nrays, uint16_t* hbar, float* at_wt, void* stream);

/* ---- one attention round in ONE launch (round 7, csrc/attend_units.hip): cpn_local_units(mode) followed by
 * cpn_attend_hidden(logits = ...) for the rays [ray0, ray0 + nrays), bit for bit, with the logit arithmetic of one ray group (4
 * adjacent rays) running under the hid stream of another (wave-specialised persistent workgroups, hand-over through LDS).
 * Replaces CoPoNeRF.py:408, 446, 450-461 (mode 0, round 1) and :472-485 (mode 2, round 2).
 *   mode, loc8 .. kh_u, lv_u: as cpn_local_units (no ce_u: mode 0 stores no coords_embed).  hid, hbar, at_wt (or NULL): as
 *   cpn_attend_hidden.  logits (nrays*V*S) fp32 or NULL: when given, the raw row dot products cpn_local_units would have stored
 *   (before the / 11.31; what cpn_logit_guard reads) are stored as well.
 *   V*S is bounded by the CU's LDS: the layer-2 weights (73 / 81 KiB) + 3 x 4 rays x V*S floats must fit 160 KiB
 *   (V*S <= 1 856 in mode 0, <= 1 684 in mode 2; CPN_E_SHAPE beyond).                                                       */
int cpn_attend_units(int mode, const float* loc8, const float* coords9, const float* w1, int ldw1, const float* b1,
                     const float* add, const uint16_t* w2, int ldw2, const float* b2, const uint16_t* wk2, int ldwk2,
                     const float* bk2, const float* w1b, int ldw1b, const float* b1b, const uint16_t* kh_u, const uint16_t* hid,
                     int B, int V, int R, int S, int ray0, int nrays, const float* lv_u, uint16_t* hbar, float* at_wt,
                     float* logits, void* stream);

/* ---- K5: exact-fp32 per-ray linear layer (MFMA 16x16x4 f32)  Y = act_out( act_in(X) . W^T + bias + res ) --
 * replaces nn.Conv1d encode_latent (CoPoNeRF.py:468) and lightfield.ResnetFC (models/lightfield.py:131-167).
 *   X (M, ldx), W (N, ldw), bias (N) or NULL, res (M, ldr) or NULL, Y (M, ldy); N <= 128; K multiple of 16     */
int cpn_linear_f32(const float* X, int ldx, const float* W, int ldw, const float* bias, const float* res, int ldr,
                   float* Y, int ldy, int M, int N, int K, int relu_in, int relu_out, void* stream);

/* ---- the light-field decoder with the output masking, ONE launch (round 3) ---------------------------------
 * replaces lightfield.ResnetFC.forward (models/lightfield.py:131-167; ResnetBlockFC :52-61) on
 * [coords of view 0 | coords of view 1 | z_local ; z_local] (models/CoPoNeRF.py:547-560) and the white background of
 * rays no context view sees (:562-566).  Exact fp32 (v_mfma_f32_16x16x4_f32), same operation order as the
 * layer-by-layer cpn_linear_f32 chain + masking pass it superseded on the inference path.
 *   coords9 (N,R,9)   z_local (B*R,416)   overlaps (N,R) uint8
 *   wpack: every weight matrix W[N][K] in MFMA FRAGMENT order (round 4) - [N/16][K/16][64 lanes][4]: lane l of fragment
 *          (t, kb) holds W[16 t + (l & 15)][16 kb + 4 (l >> 4) .. +4], so that a wave's load of one fragment is 1 KiB of
 *          contiguous memory (row-major weights read in that layout cost 64 L1 tag look-ups per instruction) - biases plain:
 *          CPN_LIGHTFIELD_PACK_FLOATS floats = lin_in W[128][32] (18 columns used, rest zero) b[128] |
 *          3 x { lin_z W[128][416] (the two 416-column halves of the reference's 832 summed) b[128] |
 *                fc_0 W[128][128] b[128] | fc_1 W[128][128] b[128] } | lin_out W[16][128] (rows 3.. zero) b[16]
 *   rgb (B,1,R,3)   valid (B,R,1) float 0/1   rgb_raw (B*R,3) or NULL: the decoder output before masking        */
#define CPN_LIGHTFIELD_PACK_FLOATS (128 * 32 + 128 + 3 * (128 * 416 + 128 + 2 * (128 * 128 + 128)) + 16 * 128 + 16)
int cpn_lightfield_decode(const float* coords9, const float* z_local, const float* wpack, const uint8_t* overlaps,
                          int B, int V, int R, float* rgb, float* valid, float* rgb_raw, void* stream);

/* ---- auxiliary per-ray outputs, ONE launch (round 3) -----------------------------------------------------
 * replaces models/CoPoNeRF.py:493-541: at_wt.argmax, the attention-weighted expected 3-D point
 * (clamp(pt,-100,100), summed over samples and views), its depth in the query camera
 * (utils_training/geometry.py:395-406), batch_project_to_other_img into both context views
 * (utils_training/utils.py:140-170), generate_mask_from_confidence_score (:260-276) and flow2kps (:52-69).
 *   at_wt (N,R,S)   pt (N,R,S,3)   uv: pixel (x,y) of ray r of pair b at uv[b*uv_batch_stride + 2 r]
 *   rayc (B, CPN_RAYC_STRIDE): row 2 of inv(query cam2world) (4) | inv(K_query[:3,:3]) (9) | K_ctx0 (9) | K_ctx1 (9) |
 *        Tq[:,0] (16) | Tq[:,1] (16)      (O(B) host pose algebra, like the camera block)
 *   mask2 (B,256,256) uint8/bool: cycle-consistency mask of view 2; flow_up (B,2,256,256): flow[1] at 256x256
 *   at_wt_max (N,R) int64   depth_ray (B,R) clamped to [0,10]   t_to_c1, t_to_c2, c2_to_c1 (B,R,2)
 *   mask_c2, match_mask (B,R) uint8 0/1                                                                         */
#define CPN_RAYC_STRIDE 64
int cpn_ray_outputs(const float* at_wt, const float* pt, const float* uv, long long uv_batch_stride, const float* rayc,
                    const uint8_t* mask2, const float* flow_up, int B, int V, int R, int S, long long* at_wt_max,
                    float* depth_ray, float* t_to_c1, float* t_to_c2, uint8_t* mask_c2, uint8_t* match_mask,
                    float* c2_to_c1, void* stream);

/* ==== the reference-arithmetic mode in the restructured formulation (csrc/encode_f32.hip, round 6) ==================
 * RenderEngine.precision = "f32": fp32 node tables, fp32 blends and products; the hidden activations are carried as fp16
 * (hi, lo) pairs - hs (rows, 3328) fp16 = [hi_own 832 | hi_other 832 | lo_own 832 | lo_other 832], x = hi + lo to 22 bits -
 * so that the folded key layer runs on cpn_gemm_f16 against (hi, lo) weights with exact products
 * (C = [hi | lo] . [W_hi | W_hi]^T, then C += hi . W_lo^T: cpn_gemm_f16 with out_f32 = 2 accumulates onto C).              */

/* the three coarse levels (NHWC fp32 maps (nimg, H/16.., 256)) sampled at every table node (grid_sample semantics of the
 * node's table: 'border' / 'zeros', models/CoPoNeRF.py:312, 370) -> feat (nimg * cpn_encode_table_nodes, 768) fp32         */
int cpn_node_features_f32(const float* map0, const float* map1, const float* map2, int H, int W, int nimg, float* feat,
                          void* stream);

/* first encoder layer on fp32 tables: per sample row (ray, view, sample, image j)
 *   hid = ReLU(sum_t a_t tab[node_t] + W[:, 768:835] . [bilinear(map3) 64 | tanh(pt/5) 3] + b)     (CoPoNeRF.py:384-397)
 * tab (nimg * nodes, 832) fp32 = node features . W[:, :768]^T, map3 (nimg, H, W, 64) fp32 NHWC, w80t (68, 832) fp32 = the
 * layer's columns 768..834 transposed (k-major) with the bias as row 67; output hs (nrays*V*S, 3328) fp16 (hi, lo) pairs.
 * hid must stay below the fp16 range (< 65 520): hi = fp16(hid) is inf beyond it and the pair no longer holds the value.   */
int cpn_encode_hidden_f32(const float* tab, const float* map3, int H, int W, const float* pixel_val, const float* sec_grid,
                          const float* pe6, const float* w80t, int B, int V, int R, int S, int ray0, int nrays, uint16_t* hs,
                          void* stream);

/* joint softmax over the V*S samples of a ray of <qa, qb> / 11.31 (fp32 (rows,128) operands) and the weighted sum of the
 * hidden activations hs (hi, lo pairs) -> hbar (nrays, 1664) fp32, at_wt (N,R,S) fp32 or NULL   (CoPoNeRF.py:450-461, 475-485) */
int cpn_attend_hidden_f32(const float* qa, const float* qb, const uint16_t* hs, int B, int V, int R, int S, int ray0, int nrays,
                          float* hbar, float* at_wt, void* stream);

/* ==== precision = "auto": a per-ray logit guard picks the rays the reference-arithmetic path re-renders (csrc/guard.hip) ====
 * The fp16 default forms the attention logits from fp16 operands (relative error ~3e-4); a softmax weight is then off by
 * ~w (1 - w) |l| 3e-4, which flat rays average away and sharp rays do not (CoPoNeRF.py:450-461, 475-485).  Under
 * |dl_i| <= eps |l_i| both sum_i |dw_i| and max_i |dw_i| are bounded by 2 eps sum_i w_i (1 - w_i) |l_i|: that sum is the
 * ray's score.                                                                                                              */

/* score of every ray of a chunk from the logits cpn_local_units stored (the layout cpn_attend_hidden reads): l_i = lg_i / 11.31,
 * w = softmax(l) formed exactly as cpn_attend_hidden forms it, score[b*R + r] = sum_i w_i (1 - w_i) |l_i| for the rays
 * [ray0, ray0 + nrays);
 * accumulate = 1: score = max(score, that) (round 2 after round 1)
 *   logits (nrays*V*S) fp32   score (B*R) fp32                                                                          */
int cpn_logit_guard(const float* logits, int B, int V, int R, int S, int ray0, int nrays, float* score, int accumulate,
                    void* stream);

/* indices of the rays with score > tau in ascending order (a deterministic scan, no atomics) and their count
 *   score (nray) fp32   list (nray) int32: entries [0, count) written   count (1) int32                                */
int cpn_select_rays(const float* score, int nray, float tau, int* list, int* count, void* stream);

/* cpn_encode_hidden_f32 / cpn_attend_hidden_f32 over a LIST of rays: local ray t of the launch is rays[ray0 + t] instead of
 * ray0 + t (rays (>= ray0 + nrays) int32, each in [0, B*R); entries outside are skipped).  hs and hbar rows are compact
 * (local ray order); at_wt is written at the listed ray's own (n, r, s) position.  Same arithmetic, bit for bit.      */
int cpn_encode_hidden_f32_rays(const float* tab, const float* map3, int H, int W, const float* pixel_val, const float* sec_grid,
                               const float* pe6, const float* w80t, int B, int V, int R, int S, const int* rays, int ray0,
                               int nrays, uint16_t* hs, void* stream);
int cpn_attend_hidden_f32_rays(const float* qa, const float* qb, const uint16_t* hs, int B, int V, int R, int S,
                               const int* rays, int ray0, int nrays, float* hbar, float* at_wt, void* stream);

/* ==== training: backward of the two non-GEMM stages (plain GEMM gradients use hipBLASLt via torch.matmul) ==== */

/* gradient of cpn_attend_hidden: dhbar (rays,1664) fp32, dw_ext (N,R,S) fp32 or NULL (external gradient on the
 * softmax weights), at_wt (N,R,S) the forward weights -> dqa, dqb (rays*V*S,128) fp16, dhid (rays*V*S,1664) fp16 or
 * NULL (the caller then forms the hidden-activation gradient of all consumers with cpn_hid_grad_combine).
 * dqb_acc (rays*V*S,128) fp16 or NULL: added to dqb (qb = coords_embed feeds both attention rounds, models/CoPoNeRF.py:450,475:
 * the second call sums the two gradients instead of autograd adding two 0.5 GB tensors)                            */
int cpn_attend_hidden_bwd(const uint16_t* qa, const uint16_t* qb, const uint16_t* hid, const float* at_wt,
                          const float* dhbar, const float* dw_ext, int B, int V, int R, int S, int ray0, int nrays,
                          uint16_t* dqa, uint16_t* dqb, uint16_t* dhid, const uint16_t* dqb_acc, void* stream);

/* gradient of cpn_attend_hidden_f32 (train_precision = "f32"): autograd's backward of the joint softmax over the 2 S samples
 * of a ray and of the attention-weighted sum, models/CoPoNeRF.py:450-461 (round 1) and 475-485 (round 2) under
 * wrapper.py:138, evaluated on the hidden activations as cpn_attend_hidden_f32 evaluates the forward.
 * qa, qb (rays*V*S,128) fp32, hs (rays*V*S,3328) fp16 = [hi_own | hi_other | lo_own | lo_other] (cpn_encode_hidden_f32),
 * at_wt (N,R,S) the forward weights, dhbar (rays,1664) fp32, dw_ext (N,R,S) fp32 or NULL -> dqa, dqb (rays*V*S,128) fp32,
 * all in fp32: dw = <hi + lo, dhbar> + dw_ext, dl = w (dw - sum w dw) / 11.31, dqa = dl qb, dqb = dl qa (+ dqb_acc).
 * dqb_acc (rays*V*S,128) fp32 or NULL: the other round's gradient of the shared qb (coords_embed), summed in.  hs's own
 * gradient w (x) dhbar is left to cpn_gemm_f16_combine_hs.  Operands 16-byte aligned.                                   */
int cpn_attend_hidden_bwd_f32(const float* qa, const float* qb, const uint16_t* hs, const float* at_wt, const float* dhbar,
                              const float* dw_ext, int B, int V, int R, int S, int ray0, int nrays, float* dqa, float* dqb,
                              const float* dqb_acc, void* stream);

/* gradient w.r.t. the pre-activation of the first encoder layer from ALL consumers of hid, in one pass:
 *   out[row,c] = hid[row,c] > 0 ? dkey[row,c] + w1[n,r,s]*dh1[ray, j*832+c] + w2[n,r,s]*dh2[ray, j*832+c] : 0
 * dkey (rows, 832) fp16 or NULL = gradient through the key path; (w_i (N,R,S) fp32, dh_i (rays,1664) fp32) or NULL =
 * the attention-weighted hidden sums (w_i: forward softmax weights, dh_i: gradient of the summed vector).            */
int cpn_hid_grad_combine(const uint16_t* dkey, const uint16_t* hid, const float* w1, const float* dh1, const float* w2,
                         const float* dh2, int B, int V, int R, int S, int ray0, int nrays, uint16_t* out, void* stream);

/* the same result WITHOUT the stored key-path gradient (round 6): the data-gradient GEMM of the folded key map
 * (autograd's grad_input of Conv2d 1664->128, models/CoPoNeRF.py:404 under wrapper.py:138) with cpn_hid_grad_combine as its
 * epilogue,   out (rows,1664) = mask(hid) . (dkh (rows,K) . Wt (1664,K)^T + w1 (x) dh1 + w2 (x) dh2),   rows = nrays*V*S.
 * dkh fp16 (row stride lda), Wt fp16 = the folded key-map weight transposed (K-contiguous rows, stride ldw), K % 32 == 0,
 * S % 16 == 0.  Same arithmetic as cpn_gemm_f16 followed by cpn_hid_grad_combine (bit-identical), 14 GB less HBM traffic
 * per training step at 4 x 4096 rays.                                                                                     */
int cpn_gemm_f16_combine(const uint16_t* dkh, int lda, const uint16_t* Wt, int ldw, const uint16_t* hid, const float* w1,
                         const float* dh1, const float* w2, const float* dh2, int B, int V, int R, int S, int ray0,
                         int nrays, int K, uint16_t* out, void* stream);

/* cpn_gemm_f16_combine with the mask read from the hi half of hs (rows, 3328) of cpn_encode_hidden_f32 (train_precision =
 * "f32"): the data gradient of the folded key layer (models/CoPoNeRF.py:404-408 under wrapper.py:138, kh = ReLU(W' (hi + lo)
 * + c')) plus the parked parts of the two attention sums (:450-461, 475-485), masked by hi > 0.  For a ReLU output hi > 0
 * <=> hi + lo > 0 except below fp16's smallest subnormal.  out (rows, 1664) fp16, the layout of cpn_gemm_f16_combine;
 * bit-identical to it run on a contiguous copy of the hi half.                                                             */
int cpn_gemm_f16_combine_hs(const uint16_t* dkh, int lda, const uint16_t* Wt, int ldw, const uint16_t* hs, const float* w1,
                            const float* dh1, const float* w2, const float* dh2, int B, int V, int R, int S, int ray0,
                            int nrays, int K, uint16_t* out, void* stream);

/* data gradient THROUGH a ReLU in one kernel:  out (M,N) fp16 = mask (M,N) > 0 ? A (M,K) . Wt (N,K)^T : 0  — grad_input of a
 * 1x1 Conv2d whose input `mask` is a ReLU output (key_map -> ReLU -> key_map_2, models/CoPoNeRF.py:404-408: autograd's
 * threshold_backward pass over the (rows,128) gradient is gone).  M %% 16 == 0, K %% 32 == 0, N %% 208 == 0 or N %% 128 == 0. */
int cpn_gemm_f16_masked(const uint16_t* A, int lda, const uint16_t* Wt, int ldw, const uint16_t* mask, int ldm, uint16_t* out,
                        int ldc, int M, int N, int K, void* stream);

/* weight gradients of the 128-wide per-sample layers (torch.mm(dY.t(), X) in the reference's autograd, i.e. the
 * Conv2d(128->128,1x1) / Conv2d(16->128,1x1) layers of models/CoPoNeRF.py:82,85-86,95-96 under wrapper.py:138):
 *   dW (128,128) fp32 += dY^T . X,  db (128) fp32 += column sums of dY (or NULL);  dY (M,128) fp16, X (M,ldx) fp16 of
 *   which the first 128 columns are used.  Both outputs are accumulated: the caller zeroes them.                      */
int cpn_wgrad_skinny_f16(const uint16_t* dY, const uint16_t* X, int ldx, long long M, float* dW, float* db, void* stream);
/* weight gradient of the 832-wide first encoder layer (dW of query_encode_latent, models/CoPoNeRF.py:437-438 under autograd):
 *   dW (N, K) fp32 = dY^T . X / scale[0]  (scale NULL -> 1), written;  dY (M, ldy) fp16 of which N columns are used, X (M, ldx)
 *   fp16 of which K columns are used;  N % 208 == 0, K % 128 == 0 (832 x 896 on the render path), 16-byte aligned rows.
 *   part: cpn_wgrad_tall_scratch(N, K) floats (per-row-slab partial sums, added in a fixed order: deterministic).        */
long long cpn_wgrad_tall_scratch(int N, int K);
int cpn_wgrad_tall_f16(const uint16_t* dY, int ldy, const uint16_t* X, int ldx, long long M, int N, int K, const float* scale,
                       float* part, float* dW, void* stream);
/* backward of cpn_local_hidden in one pass: ds, out (rows,128) fp16 (incoming gradient carrying `scale[0]`, a device
 * scalar, and the forward output for the ReLU mask), loc8 / coords9 as in the forward -> dW (128,16), db (128) fp32
 * ACCUMULATED (caller zeroes), dadd (B*R,128) fp32 written (per-ray sum, NULL when the layer had no `add`).          */
int cpn_local_hidden_bwd(const uint16_t* ds, const uint16_t* out, const float* loc8, const float* coords9,
                         const float* scale, int B, int V, int R, int S, float* dW, float* db, float* dadd, void* stream);

/* gradient of the bilinear gather of the full-resolution level w.r.t. its map (F.grid_sample backward, CoPoNeRF.py:312, 370;
 * no coordinate gradient, :380-381): the level's 64 gradient columns start at column col0 of dxin (rows, ldx) fp16; dmap3
 * (N,H,W,64) fp32 NHWC accumulated (caller zeroes); chunk_boxes: scratch of B*V*cpn_gather_bwd_chunks(R,S)*16 int32.     */
long long cpn_gather_bwd_chunks(int R, int S);
int cpn_gather_rows_bwd_level3(const uint16_t* dxin, int ldx, int col0, int H, int W, const float* pixel_val,
                               const float* sec_grid, int B, int V, int R, int S, int ray0, int nrays, float* dmap3,
                               int32_t* chunk_boxes, void* stream);

/* ---- backward of the first encoder layer in its table form (round 3, csrc/encode_bwd.hip) ---------------------------------
 * The layer is hid = ReLU(sum_t a_t T[node_t] + W[:,768:835].[gather_3 | tanh(pt/5)] + b) with T = node_features . W[:,:768]^T
 * (replaces autograd through models/CoPoNeRF.py:312, 370, 384-397 for training).  d (rows, ldx >= 832) fp16 = gradient
 * of the pre-activation (ReLU mask applied, carrying the pass's power-of-two scale).
 *   cpn_scatter_rows_tables: dtab (N * cpn_encode_table_nodes(H,W), 832) fp32, ZERO on entry, += a_t * d[row] at the four
 *       nodes of every row (own image -> border table, other image -> zeros table; the taps of cpn_encode_key).
 *       scratch: cpn_scatter_tables_scratch(H,W,B,V,R,S) int32, 16-byte aligned (bucket counters, work list and one
 *       16-byte descriptor per (row, tile it touches): the rows are counting-sorted by 8x4-node tile first).
 *   cpn_node_features_bwd: adjoint of cpn_node_features: dfeat (nodes, 768) fp32 -> dmap0..2 (N,h,w,256) fp32 NHWC,
 *       OVERWRITTEN (every texel is written once: a gather over the nodes whose footprint holds it, no atomics).
 *   cpn_gather_tail: xt (rows, 128) fp16 = [bilinear gather of the full-resolution map (64) | tanh(pt/5) (3) | 1 | 0 x 60],
 *       the K = 80 operand of the forward kernel with a ones column for the bias gradient.
 *   cpn_scale_to_f16: y = fp16(x * s) with s = 2^floor(log2(target / max|x|)) clamped to [2^-40, 2^40] found on the device and
 *       written to scale_out[0], 1 / s to scale_out[1] (TWO floats; the table gradient sums up to thousands of rows per node:
 *       its own scale before the two fp16 GEMMs; the trunk's convolution backward scales every layer's incoming gradient
 *       this way); amax_scratch: one uint32, ZERO on entry; n % 4 == 0.                                             */
long long cpn_scatter_tables_scratch(int H, int W, int B, int V, int R, int S);
int cpn_scale_to_f16(const float* x, long long n, float target, uint32_t* amax_scratch, uint16_t* y, float* scale_out,
                     void* stream);
int cpn_scatter_rows_tables(const uint16_t* d, int ldx, int H, int W, const float* pixel_val, const float* sec_grid, int B,
                            int V, int R, int S, int ray0, int nrays, float* dtab, int32_t* scratch, void* stream);
int cpn_node_features_bwd(const float* dfeat, int H, int W, int nimg, float* dmap0, float* dmap1, float* dmap2,
                          void* stream);
int cpn_gather_tail(const uint16_t* map3, int H, int W, const float* pixel_val, const float* sec_grid, const float* pe6,
                    int B, int V, int R, int S, int ray0, int nrays, uint16_t* xt, void* stream);

/* ==== get_z path: the 4-D operators of UFC =========================== */

/* ---- K6: Conv4d (+ MaxPool4d when stride > 1) + GroupNorm(1 group) + ReLU in one pass --------------
 * replaces conv4d.Conv4d / MaxPool4d / Encoder4D (models/conv4d.py:7-30, 57-163) and the einops rearrange copies
 * around them.  x (B,Cin,Hq,Wq,Hs,Ws) fp32; wq/ws (Cout,Cin,k,k), bq/bs (Cout): query / support 2-D kernels;
 * y (B,Cout,Hq',Wq',Hs',Ws') with n' = (n + 2p - k)/s + 1; gn_w/gn_b (Cout) GroupNorm affine;
 * stats: cpn_gn_stats_doubles(B, Cout, npos') float64, ZERO on entry.  On return stats[2b], stats[2b+1] = sum / sum of
 * squares of sample b's (Cout, volume) slab; the rest is the arrival counters and per-workgroup partial pairs of the
 * deterministic reduction (the last workgroup of a sample to finish sums the partials in a fixed order: two runs give
 * the same bits).  cpn_gn_relu / cpn_gn_relu_bwd read the first 2B entries.
 * scratch: cpn_conv4d_scratch(...) floats for the pooled volumes of a strided layer (0 for stride 1; NULL = no scratch,
 * the pooling window is then re-evaluated per tap).                                                             */
long long cpn_conv4d_scratch(int B, int Cin, int Hq, int Wq, int Hs, int Ws, int s);
long long cpn_gn_stats_doubles(int B, int Cout, long long npos);
/* residual (same shape as y) or NULL: added to the block's output in the normalisation pass, y = residual + ReLU(GN(conv)) —
 * the `x + Encoder4D(...)` of models/aggregation.py:306, 347-355 without a separate add over the volume.              */
int cpn_conv4d_gn_relu(const float* x, const float* wq, const float* bq, const float* ws, const float* bs,
                       const float* gn_w, const float* gn_b, const float* residual, float eps, int B, int Cin, int Cout,
                       int Hq, int Wq, int Hs, int Ws, int k, int s, int p, float* y, double* stats, float* scratch,
                       void* stream);

/* the two halves of K6 on their own (training keeps the pre-normalisation volume; the data gradient of a stride-1
 * Conv4d is a Conv4d with flipped, transposed kernels): conv (+pool) -> y and the GroupNorm sums; y -> out           */
int cpn_conv4d(const float* x, const float* wq, const float* bq, const float* ws, const float* bs, int B, int Cin,
               int Cout, int Hq, int Wq, int Hs, int Ws, int k, int s, int p, float* y, double* stats, float* scratch,
               void* stream);
/* x (N, P, Q) fp32 -> y (N, Q, P): the (query, support) pair swap of a 4-D volume, (B,C,Hq,Wq,Hs,Ws) ->
 * (B,C,Hs,Ws,Hq,Wq) with N = B*C, P = Hq*Wq, Q = Hs*Ws (x.permute(0,1,4,5,2,3).contiguous(), models/aggregation.py:349) */
int cpn_transpose_pairs(const float* x, int N, int P, int Q, float* y, void* stream);

/* data gradient of the k3 s1 p1 Conv4d (the layer's two (Cout,Cin,3,3) filters read in place, transposed and flipped):
 * dy (B,Cout,Hq,Wq,Hs,Ws) -> dx (B,Cin,Hq,Wq,Hs,Ws); Cin % 4 == 0                                                  */
int cpn_conv4d_dgrad(const float* dy, const float* wq, const float* ws, int B, int Cout, int Cin, int Hq, int Wq, int Hs,
                     int Ws, float* dx, void* stream);
int cpn_gn_relu(const float* y, const double* stats, const float* gn_w, const float* gn_b, const float* residual, float eps,
                int B, int C, long long npos, float* out, void* stream);
/* backward of GroupNorm(1 group) + ReLU (autograd of models/conv4d.py:150-158): y pre-normalisation volume, out the
 * forward output, dout its gradient, stats the forward sums; red (B*2 + C*2) float64 scratch, zero on entry ->
 * dy (B,C,npos), dgn_w (C), dgn_b (C)                                                                              */
int cpn_gn_relu_bwd(const float* y, const float* out, const float* dout, const double* stats, const float* gn_w,
                    float eps, int B, int C, long long npos, double* red, float* dy, float* dgn_w, float* dgn_b,
                    void* stream);

/* weight gradient of ONE separable branch of a 3x3 / stride-1 / pad-1 Conv4d (autograd of models/conv4d.py:108-135):
 * x (B,Cin,G,H,W), dy (B,Cout,G,H,W), convolution over (H,W) -> dw (Cout,Cin,3,3) and db (Cout, may be NULL), both
 * overwritten.  The support branch is the call on (B,C,Hq*Wq,Hs,Ws) as stored; the query branch the call on the
 * volumes with the index pairs swapped.  Cin, Cout <= 32, H*W <= 256, W >= 4.
 * partial: scratch of cpn_conv_wgrad_scratch(Cin, Cout) floats (per-workgroup partial sums).                        */
long long cpn_conv_wgrad_scratch(int Cin, int Cout);
int cpn_conv_wgrad_planes(const float* x, const float* dy, int B, int Cin, int Cout, int G, int H, int W,
                          float* partial, float* dw, float* db, void* stream);

/* weight / bias gradient of the depthwise 3x3 / stride-1 / pad-1 convolution of the UFC feed-forward blocks
 * (DWConv, models/aggregation.py): x, dy (N,C,H,W) -> dw (C,1,3,3), db (C, may be NULL), overwritten.              */
int cpn_dwconv3x3_wgrad(const float* x, const float* dy, int N, int C, int H, int W, float* dw, float* db,
                        void* stream);

/* the same DWConv directly on the token layout x (B, H*W, C) fp32 the feed-forward blocks work in (the reference
 * transposes to (B,C,H,W) around a grouped Conv2d, aggregation.py:18-28): y = bias + w (*) x (flip = 0, forward) or the
 * data gradient w_flipped (*) dy (flip = 1, bias NULL).  w (C,9).  C % 4 == 0.  flip | 2: the exact GELU that follows the
 * DWConv in the feed-forward block (aggregation.py:180, nn.GELU()) is applied to y in the same pass (inference).       */
int cpn_dwconv3x3_tokens(const float* x, const float* w, const float* bias, int B, int H, int W, int C, int flip, float* y,
                         void* stream);
/* its weight / bias gradient: dw (C,9), db (C, may be NULL), overwritten; partial = scratch of
 * cpn_dwconv3x3_tokens_wgrad_scratch(B,H,C) floats (per-row partial sums, reduced in a fixed order)                  */
long long cpn_dwconv3x3_tokens_wgrad_scratch(int B, int H, int C);
int cpn_dwconv3x3_tokens_wgrad(const float* x, const float* dy, int B, int H, int W, int C, float* partial, float* dw,
                               float* db, void* stream);

/* dual softmax of the pose branch's cross attention (models/backbone.py:296-330), a (B,L,M) fp32:
 * f = softmax(a, dim=-1) * softmax(a, dim=-2); rstat (B,L,2) / cstat (B,M,2) receive (max, sum exp) per row / column
 * and feed the backward: da from df with srow (B,L), scol (B,M) scratch.                                            */
int cpn_dual_softmax(const float* a, int B, int L, int M, float* rstat, float* cstat, float* f, void* stream);
int cpn_dual_softmax_bwd(const float* a, const float* rstat, const float* cstat, const float* f, const float* df,
                         int B, int L, int M, float* srow, float* scol, float* da, void* stream);

/* ---- K7: cosine correlation of two token sets ------------------------------------------------------
 * replaces aggregation.correlation / correlation_token (models/aggregation.py:70-80):
 * out[b,s,t] = <src[b,s]/(|src[b,s]|+eps), trg[b,t]/(|trg[b,t]|+eps)>; src, trg (B,L,C), C % 16 == 0;
 * src_n, trg_n (B,L,C) scratch for the normalised tokens; out (B,L,L) == (B,1,h,w,h,w).                    */
int cpn_correlation(const float* src, const float* trg, int B, int L, int C, float eps,
                    float* src_n, float* trg_n, float* out, void* stream);
/* VJP of the row normalisation of K7 (training): x, y = x / (|x| + eps), dy (rows, C) fp32, C <= 1024 ->
 * dx = dy / (|x| + eps) - y (y . dy) / |x|, one launch (the stock-op form was ten per call, 26 calls per step).       */
int cpn_l2norm_rows_bwd(const float* x, const float* y, const float* dy, long long rows, int C, float eps,
                        float* dx, void* stream);

/* ---- weight / bias gradient of an fp32 Linear layer (training, round 4) ---------------------------------
 * replaces the dW = dY^T . X and db = dY.sum(0) autograd performs for torch.nn.functional.linear
 * (models/aggregation.py:200-260 projection and feed-forward layers of the cost aggregation; models/CoPoNeRF.py:468 and
 * models/lightfield.py:52-61,131-167 per-ray layers): the tokens R are the contraction index of both row-major operands.
 *   dY (R, O) row stride ldy   X (R, I) row stride ldx   ->   dW (O, I) contiguous, db (O) or NULL
 *   O, I, ldy, ldx multiples of 4, operands 16-byte aligned; exact fp32 products (v_mfma_f32_16x16x4_f32), row slabs summed
 *   in a fixed order (deterministic); scratch: cpn_wgrad_f32_scratch_floats(R, O, I) floats                              */
long long cpn_wgrad_f32_scratch_floats(long long R, int O, int I);
int cpn_wgrad_f32(const float* dY, int ldy, const float* X, int ldx, long long R, int O, int I, float* dW, float* db,
                  float* scratch, void* stream);

/* ---- the Adam update of every parameter tensor, ONE launch (training, round 4) ------------------------------
 * replaces torch.optim.Adam.step() in the reference's loop (train.py:102-105, wrapper.py:149-151): default betas / eps, no
 * weight decay, no amsgrad; fp32, the operation order of the library's fused kernel.
 *   segs: device array of CPN_ADAM_SEG_BYTES-byte records, one per tensor, little-endian:
 *         { float* param; const float* grad (NULL: tensor skipped); int64 offset of its moments in exp_avg / exp_avg_sq
 *           (multiple of 4); int32 numel; float step_size = lr / (1 - beta1^k); float 1 / sqrt(1 - beta2^k); 12 bytes pad }
 *   blocks: device array of nblocks x { int32 tensor, int32 first element }: cpn_adam_chunk() elements per block
 *   gscale: device scalar multiplied into every gradient first (the clip coefficient), or NULL
 *   gate: device scalar, 0 = skip the whole update (the finite-gradient guard of wrapper.py:44-58,147-151 without a host
 *         read), or NULL.  counts_in / counts_out (one int32 per tensor, two DIFFERENT arrays swapped by the caller every
 *         step; or both NULL): the tensors' update counts kept on the device — the kernel then forms step_size and
 *         1 / sqrt(1 - beta2^k) from counts_in[t] + 1 and `lr` itself and ignores the two floats of the record             */
#define CPN_ADAM_SEG_BYTES 48
int cpn_adam_chunk(void);
int cpn_adam_step(const void* segs, const int* blocks, int nblocks, float* exp_avg, float* exp_avg_sq,
                  const float* gscale, const float* gate, const int* counts_in, int* counts_out, double lr,
                  double beta1, double beta2, double eps, void* stream);

/* ---- K8: soft-argmax with temperature over the 4-D correlation, both directions --------------------
 * replaces aggregation.soft_argmax + softmax_with_temperature (models/aggregation.py:119-144, 555-560).
 * c (B, h*h source, h*h target); t_to_s[b,:,s] = E_{t ~ softmax_t(c[b,s,:]/beta)}[(x_t, y_t)],
 * s_to_t[b,:,t] = E_{s ~ softmax_s(c[b,:,t]/beta)}[(x_s, y_s)], coordinates linspace(-1,1,h); outputs (B,2,h,h). */
int cpn_soft_argmax_pair(const float* c, int B, int h, float beta, float* t_to_s, float* s_to_t, void* stream);
/* backward of K8: t_to_s / s_to_t are the forward outputs, g_* their gradients (B,2,h*h) -> dc (B,h*h,h*h), overwritten */
int cpn_soft_argmax_pair_bwd(const float* c, int B, int h, float beta, const float* t_to_s, const float* s_to_t,
                             const float* g_t_to_s, const float* g_s_to_t, float* dc, void* stream);

/* ---- K9: linear attention of UFCLayer.forward_attention (models/aggregation.py:84-117) ------------------------------
 * phi = ELU + 1;  out = phi(Q) . (sum_s phi(K)_s (x) V_s / L) * L / (phi(Q) . sum_s phi(K)_s + eps)
 *   q, k (B, L, H, 32) fp32;  v and out: channel_major = 0 -> (B, L, H, Dv) (feature branch),
 *   channel_major = 1 -> (B, H, Dv, L) (cost-volume branch: (B, H*Ht*Wt, fs, fs) maps as stored, no permute copies)
 *   scratch: cpn_linear_attention_scratch(B, H, Dv, nsplit) floats; nsplit = number of token ranges reduced in
 *   parallel (partials are summed in a fixed order: deterministic)                                             */
long long cpn_linear_attention_scratch(int B, int H, int Dv, int nsplit);
int cpn_linear_attention(const float* q, const float* k, const float* v, int B, int L, int H, int Dv,
                         int channel_major, float eps, int nsplit, float* scratch, float* out, void* stream);
/* VJP of K9 (autograd through models/aggregation.py:84-117 in the reference): dout has out's layout, dv has v's;
 * dq, dk (B, L, H, 32).  scratch: cpn_linear_attention_bwd_scratch(B, L, H, Dv, nsplit) floats.  All three are overwritten. */
long long cpn_linear_attention_bwd_scratch(int B, int L, int H, int Dv, int nsplit);
int cpn_linear_attention_bwd(const float* q, const float* k, const float* v, const float* dout, int B, int L, int H, int Dv,
                             int channel_major, float eps, int nsplit, float* scratch, float* dq, float* dk, float* dv,
                             void* stream);

/* ---- q / k of UFCLayer.forward_attention (models/aggregation.py:276-281) from the low-resolution projection (round 3):
 *   q | k = lin + upsample(low, fs x fs, bilinear, align_corners=True) + pos_embed
 * lin (B, fs*fs, 2d): the feature half of [q_proj | k_proj] with the biases; low (B, 2d, h, w): the cost-volume half of the
 * two projections applied at the volume's native h x w positions (a Linear layer commutes with the interpolation of
 * aggregation.py:274: 6 - 16x fewer FLOPs); pos (fs*fs, dim); d = nhead*dim.  q, k (B, fs*fs, nhead, dim).          */
int cpn_qk_assemble(const float* lin, const float* low, const float* pos, int B, int fs, int h, int w, int nhead, int dim,
                    float* q, float* k, void* stream);

/* ---- cost-volume side of UFCLayer.forward_attention at the volume's native resolution (round 3) ----------------------
 * replaces models/aggregation.py:283-297 (interpolate value_corr to fs x fs, LinearAttention, interpolate the message
 * back) and the residual of :301: out = residual + D (LinearAttention(q, k, U v_low)), formed as (D diag(Z) phi(q)) .
 * ((U^T phi(k))^T v_low) — U / D the bilinear up / down-sampling (align_corners=True), exact in real arithmetic.
 *   q, k (B, fs*fs, H, 32)   v_low, residual (may be NULL), out (B, H, hs*hs, Dv)
 *   scratch: cpn_cost_volume_attention_scratch(B, fs*fs, H, hs*hs, Dv) floats                                          */
long long cpn_cost_volume_attention_scratch(int B, int L, int H, int P, int Dv);
int cpn_cost_volume_attention(const float* q, const float* k, const float* v_low, const float* residual, int B, int fs,
                              int H, int hs, int Dv, float eps, float* scratch, float* out, void* stream);

/* ---- VJP of the strided Conv4d layers (models/conv4d.py:57-135 with stride > 1: the max-pooled branches; k3 s2 p1 on
 * 32^4 and k5 s4 p2 on 64^4 volumes in UFC.embedding / UFCLayer.feat_to_corr1,2, aggregation.py:198-199, 369-371).
 * Replaces autograd through two max_pool2d + two conv2d + their permute copies.  x (B,Cin,Hq,Wq,Hs,Ws), dy the gradient of
 * the layer's output (B,Cout,Oq,Pq,Os,Ps) BEFORE GroupNorm, wq / ws (Cout,Cin,k,k).  dx (like x) or NULL; gwq, gws
 * (Cout,Cin,k,k) and gb (Cout: the gradient of EITHER bias) or all three NULL.  Maxima are routed to the first maximum of a
 * window in scan order, NaN wins (max_pool2d's rule).  Deterministic.  scratch: cpn_conv4d_strided_bwd_scratch(...) floats.
 * Compiled for Cout = 8, Cin in {1, 2, 8}, k <= 7.                                                                                */
long long cpn_conv4d_strided_bwd_scratch(int B, int Cin, int Cout, int Hq, int Wq, int Hs, int Ws, int k, int s, int p);
int cpn_conv4d_strided_bwd(const float* x, const float* dy, const float* wq, const float* ws, int B, int Cin, int Cout,
                           int Hq, int Wq, int Hs, int Ws, int k, int s, int p, float* scratch, float* dx, float* gwq,
                           float* gws, float* gb, void* stream);

/* ---- K10: cost-volume cross attention of UFCLayer.forward_cross (models/aggregation.py:327-328) -------------------
 * corr (B, H, S, T) fp32; src_v (B, S, H, C), trg_v (B, T, H, C), C == 32
 *   src_attn (B, S, H, C) = softmax over t of corr . trg_v ;  trg_attn (B, T, H, C) = softmax over s of corr, transposed . src_v */
int cpn_cross_attention(const float* corr, const float* src_v, const float* trg_v, int B, int H, int S, int T, int C,
                        float* src_attn, float* trg_attn, void* stream);
/* VJP of K10 (autograd through models/aggregation.py:327-328): g_src / g_trg = gradients of src_attn / trg_attn (the forward
 * outputs, passed back in); dcorr (B,H,S,T), dsrc_v (B,S,H,C), dtrg_v (B,T,H,C) are written.
 * scratch: cpn_cross_attention_bwd_scratch(B, H, S, T) floats.  C == 32, S, T <= 512.                                      */
long long cpn_cross_attention_bwd_scratch(int B, int H, int S, int T);
int cpn_cross_attention_bwd(const float* corr, const float* src_v, const float* trg_v, const float* src_attn,
                            const float* trg_attn, const float* g_src, const float* g_trg, int B, int H, int S, int T, int C,
                            float* scratch, float* dcorr, float* dsrc_v, float* dtrg_v, void* stream);

/* ---- f3: conv_map, the 7x7 3 -> 64 convolution behind the full-resolution feature level (CoPoNeRF.py:69, 182-187) -----
 * rgb (N, H, W, 3) fp32 in [-1, 1] exactly as the input dict holds it; fused (rgb+1)/2, ImageNet normalisation
 * (utils_training/utils.py:247-257), zero-padded 7x7 convolution and bias.  w (64, 3, 7, 7), bias (64).
 * out_nchw (N, 64, H, W) fp32 = z[3] of get_z; out_nhwc_f16 (N, H, W, 64) fp16 or NULL: the layout the render path gathers from */
int cpn_conv_map7x7(const float* rgb, const float* w, const float* bias, int N, int H, int W, float* out_nchw,
                    uint16_t* out_nhwc_f16, void* stream);

/* ---- f3: inference BatchNorm (+ residual) (+ ReLU) of the ResNet-34 trunk (models/backbone.py:10-102; torchvision's
 * BasicBlock: bn(conv(x)), `out += identity`, relu) in one pass over an NCHW fp32 map:
 *   y = act((x - mean[c]) / sqrt(var[c] + eps) * w[c] + b[c] + res),  res (N,C,HW) or NULL, relu 0/1, HW % 4 == 0; y may be x */
int cpn_bn_act(const float* x, const float* res, const float* mean, const float* var, const float* w, const float* b,
               float eps, int N, int C, int HW, int relu, float* y, void* stream);

/* ---- f3: the deep trunk layers as split-K implicit GEMMs on the fp32 MFMA with the BatchNorm / residual / ReLU epilogue
 * (inference, round 4): replaces conv + bn (+ identity) (+ relu) of torchvision's BasicBlock in layer3 / layer4 of the
 * ResNet-34 trunk (models/backbone.py:10-102) at one or a few stereo pairs, where the library's kernels leave most CUs idle.
 *   x (N, Hin, Win, Cin) NHWC fp32, Cin % 16 == 0;  wp = cpn_pack_conv_weight(w (Cout, Cin, k, k)) = [tap][ci][co], Cout % 4 == 0
 *   k in {1, 3} (padding k / 2), stride in {1, 2};  mean / var / bn_w / bn_b (Cout), eps: inference batch norm
 *   res (N, Hout, Wout, Cout) NHWC or NULL, relu 0/1;  out_nhwc and / or out_nchw (N, Cout, Hout, Wout), at least one
 *   scratch: cpn_trunk_conv_scratch_floats(...) floats.  Exact fp32 products, fixed summation order (bit-reproducible).   */
int cpn_pack_conv_weight(const float* w, int Cout, int Cin, int ksize, float* wp, void* stream);
long long cpn_trunk_conv_scratch_floats(int N, int Hin, int Win, int Cin, int Cout, int ksize, int stride);
int cpn_trunk_conv_bn_act(const float* x, const float* wp, int N, int Hin, int Win, int Cin, int Cout, int ksize, int stride,
                          const float* mean, const float* var, const float* bn_w, const float* bn_b, float eps,
                          const float* res, int relu, float* out_nhwc, float* out_nchw, float* scratch, void* stream);

/* ---- f1: the launch-bound ends of the pose head, one launch each (inference, round 4) -----------------------------
 * cpn_pose_positional: (x^2, y^2, xy, x, y, 1) of the K^-1-normalised n x n grid (models/backbone.py:209-278) from the raw
 *   intrinsics (B, V, 4, 4) of the input dict (view 0, divided by H like CoPoNeRF.py:199-201); lin = linspace(-1, 1, n);
 *   out (B, n*n, 6), index = col * n + row.
 * cpn_pose_tail: pose_regressor[1:] -> [:, :128] -> rotation / translation regressors -> 6-D rotation -> rel_pose (B, 4, 4)
 *   (models/CoPoNeRF.py:106-126,190-206) from h512 = pose_regressor[0](pose_feat) (B, 512), BEFORE its ReLU.
 *   weights: HOST array of CPN_POSE_TAIL_TENSORS device pointers, weight then bias of each Linear in the order
 *   pose[2] (256 x 512), pose[4] (256 x 256), rotation 128->64->32->6, translation 128->64->32->3.
 *   nsplit > 0: h512 holds the chunk partials (B, 512, nsplit) of cpn_pose_gemv instead and bias0 (512) is pose[0].bias.
 * cpn_pose_gemv: pose_regressor[0] without its bias at B <= 4 rows — partial[b][o][c] = <W[o], x[b]> over chunk c of the
 *   K = (16*16 + 6) * 256 * 2 inputs (W (O, K) fp32, read once for all rows; K % 4 == 0, nsplit <= 64).                    */
#define CPN_POSE_TAIL_TENSORS 16
int cpn_pose_positional(const float* intrinsics, int B, int V, float H, const float* lin, int n, float* out, void* stream);
int cpn_pose_gemv(const float* x, const float* W, int B, int K, int O, int nsplit, float* partial, void* stream);
int cpn_pose_tail(const float* h512, int nsplit, const float* bias0, const float* const* weights, int B, float* rel_pose,
                  void* stream);

/* ---- bilinear resize, align_corners=True, of `planes` independent (h,w) fp32 images -> (H,W) ----------
 * replaces F.interpolate(..., mode='bilinear', align_corners=True) in interpolate4d / forward_attention /
 * interpolate2d_token (models/aggregation.py:49-63, 285, 293, 299).                                           */
int cpn_resize_bilinear_ac(const float* src, float* dst, long long planes, int h, int w, int H, int W, void* stream);
/* its adjoint (the VJP autograd needs): g on the (H,W) grid -> out on the (h,w) grid, gathered in a fixed order (deterministic) */
int cpn_resize_bilinear_ac_adjoint(const float* g, float* out, long long planes, int h, int w, int H, int W, void* stream);

/* ---- UFC.forward's final correlation (models/aggregation.py:549-553): mean of the three levels' correlations after
 * interpolate4d (aggregation.py:49-56: bilinear, align_corners=True, over the target pair of dims, then the source pair)
 * to the finest grid.  c0 (B,1,h0,h0,h0,h0), c1 (B,1,h1,h1,h1,h1), c2 and out (B,1,n,n,n,n) fp32; one pass, in the
 * arithmetic order of the separate resize / add / divide kernels.                                                   */
int cpn_corr_mean3(const float* c0, int h0, const float* c1, int h1, const float* c2, int n, int B, float* out,
                   void* stream);

/* ==== input pipeline: uint8 frames -> the float tensors of the input dict ========================
 * replaces the host-side square crop + `rgb.astype(np.float32) / 127.5 - 1` + query-pixel selection of
 * data/realestate10k_dataio.py:333-441 (utils_training/data_util.py:116-121).
 *   frames_u8 (B, 3, Hs, Ws, 3) uint8: context view 0, context view 1, query frame of every sample
 *   crop window rows [y0, y0+H), columns [x0, x0+W);  ray_pix (B, R) int32 = y*W + x in the cropped query frame
 *   ctx_rgb (B, 2, H, W, 3) fp32, qry_rgb (B, 1, R, 3) fp32: u8 / 127.5 - 1, bit-identical to the reference's numpy  */
int cpn_prepare_input(const uint8_t* frames_u8, int B, int Hs, int Ws, int y0, int x0, int H, int W, int R,
                      const int32_t* ray_pix, float* ctx_rgb, float* qry_rgb, void* stream);

/* ==== the flow-warp SSIM term of the training loss, both directions of every pair in 2 + 2 launches (round 8) ===========
 * replaces models/loss_function.py:19-60, 109-120 (gaussian / create_window / _ssim / SSIM and the `ssim` branch of
 * LFLoss.__call__) with utils_training/utils.py:642-671 (`warp`) inside it; the validity masks of
 * utils_training/utils.py:576-602 (get_gt_correspondence_mask) times the cycle check arrive as `mask`.
 *   item k = 2 b + d: view 1 - d of rgb (B, 2, H, W, 3) fp32 (channels last, as the input dict stores it) warped by
 *   s * bilinear(flow_d[b]) (flow_d (B, 2, h, w) fp32, align_corners=False, s = H / h = W / w in {1, 2, 4, 8}, CPN_E_SHAPE
 *   otherwise) against view d, under mask (2B, H, W) bytes (item order) and the 11-tap `window` (fp32, sigma 1.5).
 * cpn_ssim_warp writes coords (2B, 2, H, W): the fp32 sampling coordinates (ix, iy) in pixels; maps (2B, 9, H, W): per channel
 *   the mask-weighted d(1 - ssim)/d(mu1, E[x^2], E[xy]); partial: 2 * 2B * cpn_ssim_warp_blocks(H, W) floats; sums (2B, 2):
 *   (sum (1 - ssim) mask, sum mask) of every item; loss (2) and inv3den (2): per direction, over the batch as upstream
 *   normalises it: sum_b num / sum_b den / 3 and 1 / (3 sum_b den).  An empty mask gives NaN, as upstream.
 * cpn_ssim_warp_bwd: gout (2) = dL/dloss[d] and inv3den stay device scalars; gup (2B, 2, H, W) is scratch (the gradient of
 *   the upsampled flow); dflow (2B, 2, h, w) is gathered per low-resolution cell.  No atomics in either: bit-reproducible. */
int cpn_ssim_warp_blocks(int H, int W);
int cpn_ssim_warp(const float* rgb, const float* flow0, const float* flow1, const uint8_t* mask, const float* window, int B,
                  int H, int W, int h, int w, float* coords, float* maps, float* partial, float* sums, float* loss,
                  float* inv3den, void* stream);
int cpn_ssim_warp_bwd(const float* rgb, const float* coords, const float* maps, const float* window, const float* gout,
                      const float* inv3den, int B, int H, int W, int h, int w, float* gup, float* dflow, void* stream);

/* ==== the image metrics of the evaluation script, any number of images in 2 launches (round 9) ===========================
 * replaces test.py:227-229 (clamp of the prediction, both images to [0, 1]), test.py:90-91, 246-253 (img2mse, mse2psnr per
 * image) and test.py:265-268 (the two .cpu().numpy() copies and skimage.metrics.structural_similarity(win_size=11,
 * gaussian_weights=True, channel_axis=-1, data_range=1) on the host).
 *   pred, target (N, H, W, 3) fp32 in the model's range [-1, 1]; only pred is clamped, a NaN stays a NaN.
 *   out (N, 3) fp32 = mse, psnr (dB; +inf at mse 0), ssim of every image: 11-tap sigma-1.5 separable window, scipy's
 *   `reflect` boundary, C1 = 1e-4, C2 = 9e-4, the map cropped by 5 pixels on every side, mean over the channels.
 *   H, W >= 11 (CPN_E_SHAPE otherwise: skimage raises there too).  partial: cpn_image_metrics_scratch(N, H, W) floats
 *   (0 for a shape cpn_image_metrics rejects).  No atomics: bit-reproducible, and image n's values do not depend on N.      */
int cpn_image_metrics_scratch(int N, int H, int W);
int cpn_image_metrics(const float* pred, const float* target, int N, int H, int W, float* partial, float* out, void* stream);

/* ==== the training / validation log on the device: flow panels, depth colours, attention entropy (round 10) ==============
 * cpn_flow_panels replaces summary/summaries.py:163-207 (and :42-63, :74-100 inside it) minus the OpenCV contour (cpn_mask_contour, round 13): both
 *   F.interpolate(mode="bilinear") * (S / h), both cycle checks torch.norm(flow + warp(flow2, flow)).le(10), both
 *   get_gt_correspondence_mask, the per-image loop of warp((rgb + 1) * 127.5, flow) -> .cpu().numpy() ->
 *   overlay_semantic_mask(color=[255, 102, 51], alpha=0.5), for both directions and all B in ONE launch.
 *   rgb (B, 2, S, S, 3) fp32 in [-1, 1] (channels last), flow0 / flow1 (B, 2, h, h) fp32, any square S >= h (the reference
 *   hard-codes 256).  Direction d warps view 1 - d by flow_d.  warped (2, B, S, S, 3) fp32 in [0, 255]; mask (2, B, S, S)
 *   bytes: norm <= 10 and the mapping inside [0, S - 1]; overlay (2, B, S, S, 3) bytes: trunc(warped), and where the mask is
 *   false trunc(0.5 u8 + 0.5 colour).  The S x S flows are never stored.
 * cpn_depth_jet replaces summaries.py:129-133: out (n, 3) fp32 = table[trunc(fl32(fl32(d / 10) * 256))] with matplotlib's
 *   under / over / bad rules (below 0 -> entry 0, 256 or above -> entry 255, NaN -> 0 0 0); table (256, 3) fp32 on the device.
 * cpn_attention_entropy replaces summaries.py:114-117 and wrapper.py:126-130: out (1) fp32 = mean over the rows of
 *   -sum_s w log(w + 1e-5) of at_wt (rows, S) fp32, any S >= 1, read once; nan_to_zero counts a NaN row as 0 (wrapper.py:129).
 *   partial: cpn_attention_entropy_blocks(rows) floats (0 for a row count it rejects); the finish runs in float64.
 * No atomics in any of them: bit-reproducible, and an image's panels do not depend on the batch around it.                   */
int cpn_flow_panels(const float* rgb, const float* flow0, const float* flow1, int B, int S, int h, float* warped, uint8_t* mask,
                    uint8_t* overlay, void* stream);
int cpn_depth_jet(const float* depth, long long n, const float* table, float* out, void* stream);
int cpn_attention_entropy_blocks(long long rows);
int cpn_attention_entropy(const float* at_wt, long long rows, int S, int nan_to_zero, float* partial, float* out, void* stream);

/* ==== LPIPS (VGG): the two ends of the metric around the library's convolutions (round 11) ================================
 * test.py:149, 258-263 call lpips.LPIPS(net='vgg') per image and read it with .item(); the package is version='0.1',
 * lpips=True, spatial=False, normalize=False.  The symbols are additive: the ABI version stays.
 * cpn_lpips_stem replaces test.py:227-229, 258-259 (clamp of the prediction; both images through [0, 1] and back, each
 *   operation rounded to fp32), the package's ScalingLayer ((x - shift) / scale, shift -.030 -.088 -.188, scale .458 .448 .450)
 *   and conv1_1 + bias + ReLU of torchvision's vgg16().features in one launch.
 *   pred, target (N, H, W, 3) fp32 in [-1, 1], channels last; only pred is clamped, a NaN stays a NaN.  w (64, 3, 3, 3),
 *   bias (64).  out (2N, H, W, 64) fp32, channels last, predictions first.  Zero padding follows the scaling: a border tap reads
 *   0.  Exact fp32 products, bias + 27 terms in (ci, ky, kx) order: bit-reproducible.  H, W >= 16 (four pools must leave a pixel;
 *   CPN_E_SHAPE otherwise).
 * cpn_lpips_head replaces the package's normalize_tensor, (a - b)^2, the bias-free 1 x 1 `lin` layers, spatial_average and the
 *   sum over the layers, for all layers and images in 2 launches.  host_* are HOST arrays of `layers` <= CPN_LPIPS_LAYERS
 *   entries, copied into the kernel's arguments: host_feat[k] (2N, h_k, w_k, C_k) fp32 channels last, predictions first;
 *   host_lin[k] (C_k); C_k a multiple of 64 up to 512, any h_k, w_k >= 1 (CPN_E_SHAPE otherwise); all 16-byte aligned.
 *   out (N) fp32 = sum_k mean_pixels sum_c lin_k[c] (a_c - b_c)^2 with a = f_pred / (sqrt(sum_c f_pred^2) + 1e-10), b likewise
 *   from f_target; per_layer (N, CPN_LPIPS_LAYERS) fp32 or NULL: the terms of that sum (0 for a layer not given).
 *   partial: cpn_lpips_head_scratch(N, layers, host_h, host_w) floats (0 for sizes cpn_lpips_head rejects).  Every feature
 *   value is read once; the finish runs in float64.  No atomics: bit-reproducible, image n's values do not depend on N, and a
 *   NaN stays in its image.                                                                                                  */
#define CPN_LPIPS_LAYERS 5
int cpn_lpips_stem(const float* pred, const float* target, const float* w, const float* bias, int N, int H, int W, float* out,
                   void* stream);
int cpn_lpips_head_scratch(int N, int layers, const int* host_h, const int* host_w);
int cpn_lpips_head(const float* const* host_feat, const float* const* host_lin, const int* host_C, const int* host_h,
                   const int* host_w, int layers, int N, float* partial, float* out, float* per_layer, void* stream);

/* ==== LPIPS as a training term: the adjoints of the two kernels above (round 14) ========================================
 * For 32 x 32-patch LPIPS fine-tuning (the reference's loaders draw the patches with lpips=True and its loss never uses
 * them).  Gradients flow to the PREDICTION only; targets carry none.  The symbols are additive: the ABI version stays.
 * cpn_lpips_head_bwd: the adjoint of cpn_lpips_head with respect to the prediction maps, all layers and images in ONE launch.
 *   host_feat, host_lin, host_C, host_h, host_w, layers, N: as cpn_lpips_head takes them (same limits, same alignment).
 *   g (N) fp32: the gradient of each image's distance.  host_dfeat[k] (N, h_k, w_k, C_k) fp32, channels last, 16-byte aligned:
 *   written whole.  Per layer with P = h w pixels and per pixel, f the prediction's vector and t the target's:
 *     s = sqrt(sum_c f_c^2), r = 1 / (s + 1e-10f), a = f r, b likewise from t, q_c = lin_c (a_c - b_c), u_c = q_c (2 g_n / P),
 *     df_j = r u_j - ((sum_c u_c f_c) r r / s) f_j.
 *   THE RULE AT s == 0 IS THIS LIBRARY'S: df = 0 for the whole pixel.  (Autograd of normalize_tensor gives NaN there, from
 *   the root's derivative at 0; the ReLU in front of every tapped map passes no gradient to a pixel whose channels are all
 *   0, and a NaN would poison the data gradient of the convolution behind it.)  A zero vector in the target alone is no
 *   special case (b = 0).  16 lanes per pixel, 16-byte loads, every feature value of both maps read once, both sums round the
 *   16 lanes.  No atomics: bit-reproducible, and image n's gradient does not depend on N.
 * cpn_lpips_stem_bwd: the adjoint of cpn_lpips_stem with respect to pred, ONE launch.  dy (N, H, W, 64) fp32: the gradient
 *   of relu1_1 of the predictions; y (N, H, W, 64): cpn_lpips_stem's own output for them (the first N images of its `out`);
 *   pred (N, H, W, 3) and w (64, 3, 3, 3) as the forward took them; dy, y 16-byte aligned.  dpred (N, H, W, 3) fp32:
 *     dpred[ci](y, x) = [-1 <= pred <= 1] (1 / scale_ci) sum_{ky, kx} sum_co w[co, ci, ky, kx] dy'[co](y - ky + 1, x - kx + 1),
 *   dy' = dy where y_out > 0 and 0 elsewhere (a NaN y_out gives 0); taps outside the image are absent; the round trip
 *   through [0, 1] has derivative 1; the clamp's mask is torch's: inclusive bounds, exactly 0 outside them and for a NaN
 *   pred.  Per (ci, ky, kx) the 64 channels are 4 FMAs in a lane (channels 4 j .. 4 j + 3 in order) and a butterfly round 16
 *   lanes; the nine taps are then added in (ky, kx) order and the sum divided by scale_ci: a fixed order, bit-reproducible.
 *   H, W >= 16 as in the forward (CPN_E_SHAPE otherwise).                                                                  */
int cpn_lpips_head_bwd(const float* const* host_feat, const float* const* host_lin, const int* host_C, const int* host_h,
                       const int* host_w, int layers, int N, const float* g, float* const* host_dfeat, void* stream);
int cpn_lpips_stem_bwd(const float* dy, const float* y, const float* pred, const float* w, int N, int H, int W, float* dpred,
                       void* stream);

/* ==== novel views from two photos: fit the photos, the camera path, the frames (round 12) ================================
 * What a caller of test.py does by hand around forward(val=True).  The symbols are additive: the ABI version stays.
 * cpn_fit_images_u8 replaces cv2.resize (realestate10k_dataio.py:340), the centre square crop of
 *   utils_training/data_util.py:116-121 and `rgb.astype(np.float32) / 127.5 - 1` (dataio.py:353) for photos of any size.
 *   img (N, Hi, Wi, 3) bytes.  The crop is rows [Hi/2 - m/2, + side), columns [Wi/2 - m/2, + side), m = min(Hi, Wi),
 *   side = (m / 2) * 2; it is resampled to size x size, separably: output i of an axis reads the taps
 *   j in [max(trunc(c - sup + 0.5), 0), min(trunc(c + sup + 0.5), side)) with weights max(0, 1 - |j + 0.5 - c| / sup) over their
 *   sum, c = (i + 0.5) side / size, sup = max(side / size, 1) - F.interpolate(mode="bilinear", antialias=True,
 *   align_corners=False); antialias = 0 takes sup = 1 (antialias=False: the half-pixel bilinear rule of cv2.resize, in float).
 *   Image n goes to out + (n % B) * batch_stride + (n / B) * view_stride (floats) as (size, size, 3) fp32 = v / 127.5f - 1.0f
 *   of the fp32 resampled v, never rounded to a byte; side == size gives cpn_prepare_input's values bit for bit.
 *   tmp: N * size * side * 3 floats.  Tap positions and weights in float64, rounded once; fp32 sums in tap order, rows first.
 *   2 launches; at most 1024 taps per axis (CPN_E_SHAPE beyond).
 * cpn_camera_path replaces test.py:96-121 (make_circle, unused there) and the ground-truth query pose: out (K, B, 4, 4) fp32,
 *   pose k of pair b = [exp(t_k log R) | t_k p] of rel_pose[b] = [R | p] (B, 4, 4) fp32 on the device, t (K) float64 on the
 *   device, any real t_k (t_k == 0: the identity, t_k == 1: R itself).  An angle below 1e-12 gives the identity rotation; beyond
 *   a quarter turn the axis comes from the symmetric part of R.  sway > 0 adds R_k (sway cos(2 pi turns t_k),
 *   sway sin(2 pi turns t_k), 0) to the position.  float64 inside, one launch.
 * cpn_pack_frames replaces the float -> uint8 round trip of a frame on the host: rgb (B, h * w, 3) fp32 in [-1, 1] -> out
 *   (B, h, w, 3) bytes = rint(min(max((x + 1) * 127.5, 0), 255)), NaN -> 0, every operation rounded to fp32.  With depth
 *   (B, h * w) fp32 and table (256, 3) fp32 (both or neither) out is (B, h, 2 w, 3): the right half is cpn_depth_jet's lookup
 *   of depth (summaries.py:129-133) times 255, rounded the same way.  One launch.                                             */
int cpn_fit_images_u8(const uint8_t* img, int N, int B, int Hi, int Wi, int size, int antialias, float* tmp, float* out,
                      long long batch_stride, long long view_stride, void* stream);
int cpn_camera_path(const float* rel_pose, const double* t, int B, int K, double sway, double turns, float* out, void* stream);
int cpn_pack_frames(const float* rgb, const float* depth, const float* table, int B, int h, int w, uint8_t* out, void* stream);

/* ==== the validation log's drawings: epipolar panels and the mask contour (round 13) =====================================
 * The two OpenCV pieces of summary/summaries.py:img_summaries, as kernels.  The symbols are additive: the ABI version stays.
 * cpn_epipolar_lines replaces two_view_geometry (summary/inspect_epipolar_geometry.py:13-43), the epiline of every point
 *   and the end points of drawpointslines (:54-55), in float64 from the fp32 inputs as numpy forms them, in ONE launch.
 *   intrinsics (B, 2, 4, 4) fp32, rel_pose and gt_rel_pose (B, 4, 4) fp32, points (P, 2) int32 (x, y).  Kind k = 0 is the
 *   estimated pose, k = 1 the true one.  F (2, B, 3, 3) f64 = inv(K_view0[:3,:3])^T [t]x R inv(K_view1[:3,:3]) (inverses by
 *   cofactors in float64, then ROUNDED TO fp32: what np.linalg.inv returns for an fp32 matrix, and so what the reference
 *   multiplies; products left to right, terms in index order); lines (2, B, P, 3) f64 = F (x, y, 1) = (a, b, c), not scaled to
 *   a^2 + b^2 = 1 as cv2.computeCorrespondEpilines does (the end points do not depend on the scale); ends (2, B, P, 4) int32
 *   = (0, int(-c / b), W, int(-(c + a W) / b)), int() truncating toward zero; valid (2, B, P) bytes: 0 where b == 0, where a
 *   value is not finite or where an end point does not fit an int32 (its ends are written as 0).  The reference raises there
 *   and drops both images of the whole batch; here that one line is left out and everything else is drawn.
 * cpn_epipolar_panels replaces drawpointslines and inspect (:46-57, :95-112): out (2, B, S, 2 S, 3) fp32 in [0, 255], one
 *   thread per output pixel, ONE launch.  rgb (B, 2, S, S, 3) fp32 in [-1, 1].  Left half: (view 1 + 1) * 127.5 with the P
 *   discs (colour unblended); right half: (view 0 + 1) * 127.5, and 0.4 colour + 0.6 original on a pixel of a valid line
 *   (cv2.addWeighted, :105-106); every other pixel keeps its original value.  Later points and lines overwrite earlier ones.
 *   colors (P, 3) fp32; ends / valid as cpn_epipolar_lines writes them for W = S.  Coverage is this library's definition,
 *   not checked against OpenCV's rasteriser: a pixel lies on the disc of centre c iff (x - cx)^2 + (y - cy)^2 <= radius^2 in
 *   integers, and on a line iff its distance to the SEGMENT between the two integer end points is <= thickness / 2 (a
 *   capsule), decided without a square root: d = p1 - p0, w = p - p0, s = w.d; s <= 0: 4 |w|^2 <= T^2; s >= |d|^2:
 *   4 |p - p1|^2 <= T^2; otherwise 4 (w x d)^2 <= T^2 |d|^2.  Exact in int64 when both |y| <= 2^15 and S <= 4096; beyond
 *   that, up to the int32 range, the same expressions in float64.  0 <= radius, 1 <= thickness, both <= 255.
 * cpn_mask_contour replaces the contour of overlay_semantic_mask (summaries.py:65-71: cv2.findContours / drawContours,
 *   thickness 1): overlay (N, S, S, 3) bytes, mask (N, S, S) bytes (non-zero = valid), out (N, S, S, 3) bytes: (255, 102, 51)
 *   on every invalid pixel with a valid or outside-the-image 4-neighbour (the border points of 8-connected border following),
 *   the overlay's value elsewhere.  ONE launch for all N.
 * No atomics in any of them: bit-reproducible, and an image's result does not depend on the batch around it.                 */
int cpn_epipolar_lines(const float* intrinsics, const float* rel_pose, const float* gt_rel_pose, const int* points, int B, int P,
                       int W, double* F, double* lines, int* ends, uint8_t* valid, void* stream);
int cpn_epipolar_panels(const float* rgb, const int* points, const float* colors, const int* ends, const uint8_t* valid, int B,
                        int S, int P, int radius, int thickness, float* out, void* stream);
int cpn_mask_contour(const uint8_t* overlay, const uint8_t* mask, int N, int S, uint8_t* out, void* stream);

/* ==== a fused coloured point cloud from the depth of K rendered views (round 15) ========================================
 * What a caller does by hand with depth_ray (models/CoPoNeRF.py:509-540: the z-depth, in the query camera, of the 3-D point of
 * the ray's strongest sample, clamped to [0, 10]) to get geometry out of two photos.  The symbols are additive: the ABI
 * version stays.  The validity rule and the vote rule below are THIS LIBRARY'S definitions, not the reference's.
 * Shared by the first two: the pixel grid is the window (y0, x0, h, w) of an S x S image, pixel (r, c) of it is
 *   (u, v) = (x0 + c, y0 + r) and its ray ((u - cx) / fx, (v - cy) / fy, 1): batch_project_to_other_img's convention, no
 *   half-pixel offset.  intrinsics (B, 4, 4) fp32 (fx, fy, cx, cy = entries 0, 5, 2, 6), one camera model per pair for all K
 *   views; poses (K, B, 4, 4) fp32, camera to reference, rigid (cpn_camera_path's output); the inverse is [R^T | -R^T t].
 *   depth (K, B, h w) fp32; a depth is VALID iff it is finite and 0 < d < 10 - both clamp ends count as saturated.  float64
 *   from the fp32 inputs, one rounding per operation, sums left to right, ONE rounding to fp32 at the store.
 *   1 <= K <= 255, K B h w < 2^31, the window inside the grid (CPN_E_SHAPE otherwise).  One launch each, no atomics.
 * cpn_depth_points: xyz (K, B, h w, 3) fp32 = pose . (d . ray), the point in the reference frame; three NaN where d is invalid.
 * cpn_depth_votes: forward-backward consistency (the fusion rule of multi-view stereo).  For a valid pixel p of view a with
 *   X = pose_a . (d_a . ray(p)) and every other view b in ascending order:  Y = pose_b^-1 X, not consistent if Y_z <= 0;
 *   q = (fx Y_x / Y_z + cx, fy Y_y / Y_z + cy); in window coordinates (q_x - x0, q_y - y0) the four bilinear taps
 *   (floor, floor + 1 per axis) must lie inside the window and all be valid, else not consistent;
 *   d_b = bilinear(depth_b, q) (rows blended after columns), X' = pose_b . (d_b . ray(q)), Y' = pose_a^-1 X', not consistent
 *   if Y'_z <= 0; p' = proj(Y');  consistent iff |p' - p|_2 <= px_tol and |Y'_z - d_a| <= rel_tol d_a.
 *   votes (K, B, h w) bytes = the number of consistent b, 0 for an invalid pixel; depth_fused (K, B, h w) fp32 =
 *   (d_a + sum of Y'_z over the consistent b, in view order) / (1 + votes), NaN where d_a is invalid.  px_tol, rel_tol >= 0.
 * cpn_compact_points: deterministic stream compaction in TWO launches.  keep (K, B, h w) bytes (non-zero = selected), xyz
 *   (K, B, h w, 3) fp32, rgb (K, B, h w, 3) fp32 in [-1, 1] -> per pair b, with cap = K h w: out_xyz (B, cap, 3) fp32, out_rgb
 *   (B, cap, 3) bytes by cpn_pack_frames' rule (rint(min(max((x + 1) * 127.5, 0), 255)), NaN -> 0) and count (B) int32: the
 *   selected points in ascending (view, row, column) order; rows count[b] and beyond are left untouched.  A workgroup owns
 *   CPN_COMPACT_TILE consecutive elements of a pair; the first launch writes its count to scratch
 *   (cpn_compact_points_scratch(K, B, h, w) ints, 0 for a shape the kernels do not take), the second adds the counts before
 *   its own with 256 threads, CPN_COMPACT_FINISH counts per pass in a fixed order, and writes.  No atomics: two runs give the
 *   same bytes.  B <= 65535 here.                                                                                          */
#define CPN_COMPACT_TILE 1024
#define CPN_COMPACT_FINISH 256
int cpn_depth_points(const float* depth, const float* poses, const float* intrinsics, int K, int B, int S, int y0, int x0, int h,
                     int w, float* xyz, void* stream);
int cpn_depth_votes(const float* depth, const float* poses, const float* intrinsics, int K, int B, int S, int y0, int x0, int h,
                    int w, double px_tol, double rel_tol, uint8_t* votes, float* depth_fused, void* stream);
int cpn_compact_points_scratch(int K, int B, int h, int w);
int cpn_compact_points(const uint8_t* keep, const float* xyz, const float* rgb, int K, int B, int h, int w, int* scratch,
                       float* out_xyz, uint8_t* out_rgb, int* count, void* stream);

/* ==== dense correspondences from the two flows, and the pose refined against them (round 16) ============================
 * What a caller does by hand with the flows of get_z to get the matches between two photos, and to ask whether the estimated
 * pose agrees with them.  The symbols are additive: the ABI version stays.  The selection and the refinement are THIS LIBRARY'S
 * definitions, not the reference's.  Conventions:
 *   flow direction: flow0 (B, 2, h, h) fp32 lives on view 0's grid and points into view 1: p + flow0(p) is the match of p;
 *     flow1 lives on view 1's grid and points into view 0 (what cpn_soft_argmax_pair produces and cycle_masks and
 *     cpn_flow_panels consume).  Direction d = 0 is the pixels of view 0 matched into view 1 by flow0, d = 1 the other way.
 *   pose: rel_pose (B, 4, 4) fp32 = [R | t] with X0 = R X1 + t, E = [t]x R and a^T E b = 0 for the normalised points a of
 *     view 0 and b of view 1: the convention of cpn_epipolar_lines' F and of cpn_camera_path at t = 1.
 *   intrinsics (B, 2, 4, 4) fp32, a pinhole without skew per view: fx, fy, cx, cy = entries 0, 5, 2, 6; the normalised point
 *     of pixel (x, y) is ((x - cx) / fx, (y - cy) / fy, 1), no half-pixel offset (as cpn_depth_points).
 *   the Sampson residual of the pixel pair (a of view 0, b of view 1) under E, in pixels, in float64 from the fp32 inputs,
 *     one rounding per operation, sums left to right:  (E b)_i = (E_i0 b_0 + E_i1 b_1) + E_i2, (E^T a)_j likewise down the
 *     columns, E_0j = t_1 R_2j - t_2 R_1j, E_1j = t_2 R_0j - t_0 R_2j, E_2j = t_0 R_1j - t_1 R_0j;
 *     n = (a_0 (E b)_0 + a_1 (E b)_1) + (E b)_2;  g = ((E b)_0 / fx0, (E b)_1 / fy0, (E^T a)_0 / fx1, (E^T a)_1 / fy1);
 *     D = ((g_0^2 + g_1^2) + g_2^2) + g_3^2;  r = n / sqrt(D).  r does not count (NaN) where D <= 0 or n, D or r is not finite.
 * cpn_match_fields: ONE launch for both directions and all pairs, one thread per pixel p = (x, y) of the S x S grid, S a
 *   multiple of h.  u = (S / h) . F.interpolate(flow_d, S, mode="bilinear")(p) and q = p + u in fp32; inside = 0 <= q_x <= S - 1
 *   and 0 <= q_y <= S - 1 (aux_outputs._inside); w = the other direction's upsampled flow read at q as utils.warp and
 *   grid_sample (bilinear, zeros padding, align_corners=False) read it, a tap outside contributing 0;
 *   cycle = sqrt((u_x + w_x)^2 + (u_y + w_y)^2) in fp32: the value cycle_masks and cpn_flow_panels threshold at 10, in their
 *   expression sequence.  epi = the residual above rounded once to fp32, of (a, b) = (p, q) for d = 0 and (q, p) for d = 1.
 *   q (2, B, S, S, 2), cycle (2, B, S, S), epi (2, B, S, S) fp32, inside (2, B, S, S) bytes: every element is written.  A
 *   non-finite flow gives inside = 0 and a non-finite cycle and reads no tap.  1 <= B <= 32767, S <= 16384, 2 B S S < 2^31
 *   (CPN_E_SHAPE otherwise).
 * cpn_compact_matches: cpn_compact_points' deterministic TWO launches (CPN_COMPACT_TILE, CPN_COMPACT_FINISH) on matches.  keep
 *   (2, B, S, S) bytes (non-zero = kept), q, cycle, epi as above -> per pair, with cap = 2 S S: xy (B, cap, 4) fp32 =
 *   (x0, y0, x1, y1), view 0's point first whatever the direction, err (B, cap, 2) fp32 = (cycle, epi), count (B) int32; the
 *   kept matches in ascending (direction, row, column) order, rows count[b] and beyond left untouched.  scratch:
 *   cpn_compact_matches_scratch(B, S) ints (0 for a shape the kernels do not take).  No atomics: two runs, the same bytes.
 * cpn_refine_pose: robust Gauss-Newton on the residuals of the matches, ONE launch, one workgroup per pair.  xy (B, N, 4) fp32
 *   with count (B) int32 on the device (rows beyond min(max(count, 0), N) are never read), iters >= 0, scale_px > 0.  State per
 *   pair, float64: R and a unit t from rel_pose, t = t0 / |t0|.  Pass k = 0, 1, ..: every match i whose residual r_i counts
 *   adds, with J_ik = dn / sqrt(D) - (n dD) / ((2 D) sqrt(D)) for the six parameters (w: R <- exp([w]x) R; then dt),
 *   dE_k = [t]x [e_k]x R (k < 3) and [e_(k-3)]x R, dn = a^T dE_k b, dD = 2 (((g_0 (dE_k b)_0 / fx0 + g_1 (dE_k b)_1 / fy0) +
 *   g_2 (dE_k^T a)_0 / fx1) + g_3 (dE_k^T a)_1 / fy1), and the weight w_i = 1 / u^2, u = 1 + (r_i / scale_px)^2:
 *   H_jk += (w_i J_ij) J_ik (j <= k), g_j += (w_i J_ij) r_i, cost += ((r_i r_i) / 2) / u, sum w, the number of matches that
 *   count.  Thread t adds the matches t, t + 256, .. in ascending order; the 64 lanes of a wave by the xor butterfly 32 .. 1; the
 *   four waves as (0 + 1) + (2 + 3).  While k < iters: A = H, A_jj = H_jj + 1e-3 H_jj, the translation block
 *   += (tr H / 6) t t^T (the gauge: the residual cannot see the length of t); delta = -A^-1 g by Cholesky; a pivot <= 0 or a
 *   value that is not finite leaves the state as it is, sets status 1 and ends the pair's passes.  Otherwise
 *   R <- exp([delta_w]x) R by Rodrigues (the identity below an angle of 1e-12), t <- (t + delta_t) / |t + delta_t|.
 *   pose (B, 4, 4) fp32 = [R | |t0| t], last row 0 0 0 1: the translation keeps the length it came with.  stats (B, 8) f64:
 *   the cost of pass 0; the cost, the sum of weights and the number of matches that count of the last pass (the state that is
 *   returned); the angles in degrees between R and rel_pose's rotation (2 asin(|R - R0|_F / (2 sqrt 2))) and between t and
 *   t0 / |t0| (2 asin(|t - t0 / |t0|| / 2)); the updates made; status: 0 ok, 1 a failed solve, 2 nothing to do (count <= 0,
 *   |t0| == 0, a non-finite pose or iters == 0): then pose is rel_pose's 16 values and the other seven stats are 0.
 *   No atomics: bit-reproducible, and a pair's result does not depend on the batch around it.                               */
int cpn_match_fields(const float* flow0, const float* flow1, const float* intrinsics, const float* rel_pose, int B, int S, int h,
                     float* q, float* cycle, float* epi, uint8_t* inside, void* stream);
int cpn_compact_matches_scratch(int B, int S);
int cpn_compact_matches(const uint8_t* keep, const float* q, const float* cycle, const float* epi, int B, int S, int* scratch,
                        float* xy, float* err, int* count, void* stream);
int cpn_refine_pose(const float* xy, const int* count, const float* intrinsics, const float* rel_pose, int B, int N, int iters,
                    double scale_px, float* pose, double* stats, void* stream);

/* ==== z-buffered views of a point cloud, and their score against a photo (round 17) ======================================
 * What a caller does with a viewer on another machine to look at cpn_compact_points' cloud, and a check of depth and pose
 * against a photo that needs no ground truth.  The symbols are additive: the ABI version stays.  The footprint, the fill and
 * the tie rule below are THIS LIBRARY'S definitions: there is no perspective-sized point, no blending and no antialiasing.
 * Conventions (cpn_depth_points'): xyz (B, cap, 3) fp32 in the reference frame, rgb (B, cap, 3) bytes, count (B) int32 on the
 *   device - rows beyond min(max(count[b], 0), cap) are never read; poses (K, B, 4, 4) fp32, camera to reference, rigid: the
 *   inverse is [R^T | -R^T t]; intrinsics (B, 4, 4) fp32 of the OUTPUT image (fx, fy, cx, cy = entries 0, 5, 2, 6), no
 *   half-pixel offset: pixel (r, c) is (u, v) = (c, r).  The output image is H x W, whatever grid the cloud came from.
 *   float64 from the fp32 inputs, one rounding per operation, sums left to right.  1 <= K <= 255, K B H W < 2^31, 1 <= cap and
 *   K B ceil(cap / 256) < 2^31 (CPN_E_SHAPE otherwise).
 * cpn_splat_points: zbuf (K, B, H, W) uint64.  Every key is first set to all-ones (hipMemsetAsync), then ONE launch over
 *   (camera k, pair b, point i).  With X the point and [R | t] the pose (k, b):
 *   Y_j = (R_0j (X_0 - t_0) + R_1j (X_1 - t_1)) + R_2j (X_2 - t_2).  The point COUNTS iff X, the twelve entries of [R | t] and
 *   fx, fy, cx, cy are finite, Y_z >= near (near > 0), u = (fx Y_x) / Y_z + cx and v = (fy Y_y) / Y_z + cy are finite and
 *   below 2^30 in magnitude, and z32 = (float)Y_z is finite.  Its pixel is (c, r) = (floor(u + 0.5), floor(v + 0.5)), its
 *   footprint the (2 radius + 1)^2 square of pixels around it, clipped to the image (0 <= radius <= 8), its key
 *   (bits of z32) << 32 | i: the bit patterns of non-negative floats are ordered as their values, and of two points of equal
 *   z32 the one of the lower index has the smaller key.  Every pixel of the footprint takes the minimum of its key and the
 *   point's by a 64-bit unsigned integer atomic minimum.  This is the library's one atomic on a result path, and it keeps the
 *   rule that two runs give the same bytes: the minimum of a set of integers does not depend on the order in which they arrive.
 *   (A key that is read as already smaller than the point's skips the atomic: keys only decrease.)
 * cpn_splat_resolve: ONE launch, one thread per output pixel.  The pixel's key is its own; if that is all-ones and fill > 0 it
 *   is the smallest key of the (2 fill + 1)^2 neighbourhood of zbuf as cpn_splat_points left it, clipped to the image: holes
 *   are filled from splatted pixels only, never from filled ones (0 <= fill <= 4).  A pixel is EMPTY if that key is all-ones
 *   (or its low word is not below cap: no point wrote it).  index (K, B, H, W) int32 = the low word, -1 if empty; depth
 *   (K, B, H, W) fp32 = the float of the high word, NaN if empty; frames (K, B, H, W, 3) bytes = rgb[b, index], or the bytes
 *   (background, background >> 8, background >> 16) & 255 if empty (0 <= background < 2^24).  Every element of the three is
 *   written; depth and index may be null.
 * cpn_splat_score: frames and target (K, B, H, W, 3) bytes, index (K, B, H, W) int32 -> stats (K, B, 2) int64: n, the number of
 *   pixels with index >= 0, and the sum over those pixels and their three channels of (frame - target)^2.  Integers, so exact
 *   in any order, without atomics: a workgroup of the first launch adds CPN_SPLAT_SCORE_TILE pixels of one image into scratch
 *   (cpn_splat_score_scratch(K, B, H, W) int64 values, 0 for a shape the kernels do not take), the second adds an image's
 *   workgroups.  Two launches.                                                                                             */
#define CPN_SPLAT_SCORE_TILE 4096
int cpn_splat_points(const float* xyz, const int* count, const float* poses, const float* intrinsics, int K, int B, int cap, int H,
                     int W, int radius, double near, unsigned long long* zbuf, void* stream);
int cpn_splat_resolve(const unsigned long long* zbuf, const uint8_t* rgb, int K, int B, int cap, int H, int W, int fill,
                      int background, uint8_t* frames, float* depth, int* index, void* stream);
int cpn_splat_score_scratch(int K, int B, int H, int W);
int cpn_splat_score(const uint8_t* frames, const int* index, const uint8_t* target, int K, int B, int H, int W, long long* scratch,
                    long long* stats, void* stream);

/* ==== TSDF fusion of the rendered depth maps and a surface-nets mesh (round 18) ===========================================
 * What a caller does with a fusion library on another machine to get a SURFACE out of render_path's K depth maps: a depth map
 * is a staircase (depth_ray is the depth of one of 2 x 64 samples), and a truncated signed distance averaged per voxel over
 * the views places the surface between the steps.  The symbols are additive: the ABI version stays.  The integration rule, the
 * vertex rule and the observed-cell rule below are THIS LIBRARY'S definitions.
 * Conventions are cpn_depth_points' and cpn_splat_points': intrinsics (B, 4, 4) fp32 (fx, fy, cx, cy = entries 0, 5, 2, 6), no
 *   half-pixel offset; poses (K, B, 4, 4) fp32, camera to reference, rigid, the inverse [R^T | -R^T t] in cpn_splat_points'
 *   expression Y_j = (R_0j (X_0 - t_0) + R_1j (X_1 - t_1)) + R_2j (X_2 - t_2); the pixel grid is the window (y0, x0, h, w) of an
 *   S x S image; depth (K, B, h w) fp32, VALID iff finite and 0 < d < 10; valid (K, B, h w) bytes (forward's valid_mask as
 *   render_path returns it), rgb (K, B, h w, 3) fp32 in [-1, 1].  float64 from the fp32 inputs, one rounding per operation, sums
 *   left to right from 0, ONE rounding to fp32 at a store; bytes by cpn_pack_frames' rule in fp32 as cpn_compact_points applies
 *   it: rint(min(max((x + 1) * 127.5, 0), 255)), NaN -> 0, x the float64 value rounded once to fp32.  1 <= K <= 255.  No atomics
 *   anywhere: two runs give the same bytes, and a pair's result does not depend on the batch around it.
 * The volume of pair b: a lattice of Nx x Ny x Nz voxels (each >= 2, host integers shared by the batch), voxel (ix, iy, iz) at
 *   X = origin[b] + (ix sx, iy sy, iz sz) in the reference frame (view 0's), X_x = o_x + ix * s_x and likewise; origin (B, 3),
 *   spacing (B, 3) and trunc (B) fp32 ON THE DEVICE.  Arrays are (B, Nz, Ny, Nx), x fastest.
 * cpn_tsdf_integrate: ONE launch, one thread per voxel, the views in ascending order inside it.  For view k: Y = pose^-1 X; the
 *   view is skipped unless Y_z > 0 and Y is finite; u = (fx Y_x) / Y_z + cx, v = (fy Y_y) / Y_z + cy,
 *   (c, r) = (floor(u + 0.5) - x0, floor(v + 0.5) - y0); skipped unless 0 <= c < w and 0 <= r < h (a NaN fails), the depth d at
 *   (r, c) is valid and the valid byte there is not 0; s = d - Y_z, the signed distance along the optical axis (depth_ray is a
 *   z-depth); skipped if s < -trunc; otherwise the view UPDATES the voxel with f = min(1, s / trunc) and the pixel's rgb.
 *   tsdf (B, Nz, Ny, Nx) fp32 = (the sum of f over the updating views) / their number n, 1 if n = 0; weight, bytes, = n; colour
 *   (B, Nz, Ny, Nx, 3) fp32 = (the sum of the updating views' rgb) / n, 0 if n = 0.  Every element of the three is written.  A
 *   pair whose trunc or any spacing entry is not finite or not > 0 gets the empty volume (weight 0, tsdf 1, colour 0).
 *   K B h w < 2^31, B Nx Ny Nz < 2^31, the window inside the grid (CPN_E_SHAPE otherwise).
 * Extraction: naive surface nets, two stages, each cpn_compact_points' deterministic TWO launches (CPN_COMPACT_TILE,
 *   CPN_COMPACT_FINISH).  INSIDE means tsdf < 0 (an exact 0, and a NaN, is outside).  Cell (cx, cy, cz), 0 <= c < N - 1, has corner
 *   i = dx + 2 dy + 4 dz at voxel (cx + dx, cy + dy, cz + dz).  It is OBSERVED iff all eight corners have weight >= min_weight
 *   (1 <= min_weight <= 255) and ACTIVE iff it is observed and its corners are neither all inside nor all outside.  Its twelve
 *   edges, as (lower corner, upper corner), in this order: the x-edges (0,1) (2,3) (4,5) (6,7), the y-edges (0,2) (1,3) (4,6)
 *   (5,7), the z-edges (0,4) (1,5) (2,6) (3,7) - each group in (0,0), (1,0), (0,1), (1,1) order of the other two offsets.
 *   1 <= B <= 65535, B cells < 2^31 and 3 B voxels < 2^31 (CPN_E_SHAPE otherwise; the _scratch functions return 0).
 * cpn_surface_vertices: the cells of a pair form one sequence in (cz, cy, cx) order, cells = (Nx-1)(Ny-1)(Nz-1) of them; every
 *   active cell gets one vertex, in that order.  Every edge (a, b) whose ends differ in INSIDE contributes its zero crossing
 *   t = f_a / (f_a - f_b) from the lower corner: the point (dx, dy, dz) of corner a with t added along the edge's axis, and the
 *   colour (1 - t) colour_a + t colour_b per channel.  p = (the sum of the points) / m and the colour (the sum of the colours) / m
 *   over the m contributing edges, in the edge order; the vertex is origin + ((cx, cy, cz) + p) * spacing per axis, rounded once
 *   to fp32, its colour the byte rule above.  vert_xyz (B, capv, 3) fp32, vert_rgb (B, capv, 3) bytes, nvert (B) int32 = the TRUE
 *   number of active cells, even above capv; rows at and beyond min(nvert, capv) are left untouched.  cell_vertex (B, cells)
 *   int32 = the vertex row of every active cell (even a row >= capv), -1 elsewhere: every element is written.  scratch:
 *   cpn_surface_vertices_scratch(B, Nx, Ny, Nz) ints.  capv >= 1.
 * cpn_surface_faces: the lattice edges of a pair form one sequence e = 3 voxel + axis, voxels in (iz, iy, ix) order.  Edge (p, a)
 *   runs from voxel p to p + e_a and EXISTS iff p_a + 1 < N_a.  With (a, b, c) the cyclic order of the axes its four cells are
 *   (p_b - 1, p_c - 1), (p_b, p_c - 1), (p_b, p_c), (p_b - 1, p_c) at p_a, their vertices v00, v10, v11, v01.  The edge is SELECTED
 *   iff it exists, its ends differ in INSIDE, the four cells lie in the lattice and all four are active (cell_vertex >= 0:
 *   cpn_surface_vertices' output, made with the same tsdf).  A selected edge writes two consecutive triangles:
 *   (v00, v10, v11), (v00, v11, v01) if the lower end p is inside, (v00, v11, v10), (v00, v01, v11) otherwise - the normals point
 *   from inside to outside, towards the cameras' free space.  faces (B, capf, 3) int32, nface (B) int32 = the TRUE number of
 *   triangles (2^31 - 1 if it is larger); rows at and beyond capf are left untouched.  scratch:
 *   cpn_surface_faces_scratch(B, Nx, Ny, Nz) ints.  capf >= 1.                                                             */
int cpn_tsdf_integrate(const float* depth, const uint8_t* valid, const float* rgb, const float* poses, const float* intrinsics,
                       const float* origin, const float* spacing, const float* trunc, int K, int B, int S, int y0, int x0, int h,
                       int w, int Nx, int Ny, int Nz, float* tsdf, uint8_t* weight, float* colour, void* stream);
int cpn_surface_vertices_scratch(int B, int Nx, int Ny, int Nz);
int cpn_surface_vertices(const float* tsdf, const uint8_t* weight, const float* colour, const float* origin, const float* spacing,
                         int B, int Nx, int Ny, int Nz, int min_weight, int capv, int* scratch, float* vert_xyz, uint8_t* vert_rgb,
                         int* nvert, int* cell_vertex, void* stream);
int cpn_surface_faces_scratch(int B, int Nx, int Ny, int Nz);
int cpn_surface_faces(const float* tsdf, const int* cell_vertex, int B, int Nx, int Ny, int Nz, int capf, int* scratch, int* faces,
                      int* nface, void* stream);

/* ==== z-buffered views of a triangle mesh (round 19) =======================================================================
 * What a caller does with a viewer on another machine to look at cpn_surface_faces' mesh: its TRIANGLES drawn into any camera, so
 * that the surface is closed where it is closed and hides what lies behind it.  The symbols are additive: the ABI version stays.
 * NO CLIPPING, the 1/256-pixel snap, the fill rule, the tie rule and the headlight below are THIS LIBRARY'S definitions; there is
 * no antialiasing, no blending, no texture and no smooth normal.
 * Conventions are cpn_splat_points', word for word: xyz (B, capv, 3) fp32 in the reference frame, rgb (B, capv, 3) bytes, nvert (B)
 *   int32 and faces (B, capf, 3) int32, nface (B) int32 on the device as cpn_surface_vertices and cpn_surface_faces leave them;
 *   poses (K, B, 4, 4) fp32, camera to reference, rigid: the inverse is [R^T | -R^T t]; intrinsics (B, 4, 4) fp32 of the OUTPUT image
 *   (fx, fy, cx, cy = entries 0, 5, 2, 6), no half-pixel offset: pixel (c, r) has its centre at (u, v) = (c, r).  float64 from the
 *   fp32 inputs, one rounding per operation, sums left to right.  1 <= K <= 255, K B H W < 2^31, 1 <= H, W <= 16384, capv, capf >= 1
 *   and K B ceil(capf / 256) < 2^31 (CPN_E_SHAPE otherwise).
 * A face f of pair b (a row of faces, 0 <= f < capf) in camera (k, b) is DRAWABLE iff all of this holds, tested in this order:
 *   the twelve entries of [R | t] and fx, fy, cx, cy are finite; each of its three indices lies in [0, min(max(nvert[b], 0), capv))
 *   (nothing is read through one that does not); each vertex X is finite; with
 *   Y_j = (R_0j (X_0 - t_0) + R_1j (X_1 - t_1)) + R_2j (X_2 - t_2), Y_z >= near, Y_z > 0 and (float)Y_z is finite AT ALL THREE
 *   VERTICES - there is no clipping: a face with one vertex nearer than near is not drawn at all; the snapped coordinates
 *   SX = floor(256 u + 0.5), SY = floor(256 v + 0.5) of u = (fx Y_x) / Y_z + cx, v = (fy Y_y) / Y_z + cy are below 2^29 in
 *   magnitude (2^21 pixels; a NaN fails), from here on int64; and the doubled area
 *   D(a, b, c) = (SX_b - SX_a)(SY_c - SY_a) - (SY_b - SY_a)(SX_c - SX_a) of its vertices in the order stored is not 0.
 *   The face is FRONT iff that D < 0: with x right, y down, z forward and fx fy > 0, D has the sign of Y_0 . ((Y_1 - Y_0) x (Y_2 - Y_0)),
 *   which is negative when the normal cpn_surface_faces winds (towards the cameras' free space) points at the camera.
 *   CANONICAL ORDER: the three vertices sorted by ascending index, then the second and third exchanged if D of that order is
 *   negative; A = |D| > 0.  Everything below uses the vertices 0, 1, 2 of this order, so no result depends on the order in which
 *   a face stores its indices (weight j of `bary` is stored at the position the vertex has in the face's row).
 *   Edge functions at the pixel centre (256 c, 256 r): w_0 = E(1, 2), w_1 = E(2, 0), w_2 = E(0, 1) with
 *   E(a, b) = (SX_b - SX_a)(256 r - SY_a) - (SY_b - SY_a)(256 c - SX_a); w_0 + w_1 + w_2 = A.  Edge a -> b OWNS the centres on it iff
 *   SY_b - SY_a < 0, or SY_b = SY_a and SX_b - SX_a > 0 (a left edge, or a top edge: the TOP-LEFT RULE).  The face COVERS the
 *   pixel iff for each edge w > 0, or w = 0 and the edge owns: a centre on an edge that two faces of a sheet share runs the two
 *   ways in them and belongs to exactly one, and so does a centre on a vertex of the sheet.
 *   q_i = (double)w_i / Y_z,i; s = (q_0 + q_1) + q_2; the depth z = (double)A / s (the perspective-correct camera z), rounded ONCE
 *   to fp32.
 * cpn_raster_faces: zbuf (K, B, H, W) uint64.  Every key is first set to all-ones (hipMemsetAsync), then ONE launch over
 *   (camera k, pair b, face f), f in [0, min(max(nface[b], 0), capf)): rows beyond are never read.  cull = 0 draws every drawable
 *   face, cull = 1 only the front ones; near > 0.  Every pixel that the face covers, of its bounding box clipped to the image,
 *   takes the minimum of its key and (bits of the fp32 depth) << 32 | f by cpn_splat_points' 64-bit unsigned atomic minimum
 *   (behind the same relaxed load): the nearest face wins, of equal fp32 depths the lower f, and two runs give the same bytes.
 *   A thread sets a face up and walks the box itself if it holds at most CPN_RASTER_SMALL pixels; the faces with larger boxes
 *   are then taken by their whole wave, one at a time, its 64 lanes striding over the box.
 *   The launch has min(ceil(capf / 256), CPN_RASTER_TILES) workgroups per (camera, pair), which stride over the pair's faces up to
 *   nface: its size depends on nothing in device memory, and its cost hardly on the room a mesh has to spare.
 * cpn_raster_resolve: ONE launch, one thread per output pixel; there is no fill pass, a triangle surface has no holes between
 *   samples.  A pixel is EMPTY if its key is all-ones or the key's low word f is not below capf or face f is not drawable with
 *   near = 0 (nothing is read for it).  Otherwise index (K, B, H, W) int32 = f; depth (K, B, H, W) fp32 = the float of the high
 *   word; bary (K, B, H, W, 3) fp32 = (float)(q_j / s); frames (K, B, H, W, 3) bytes, with byte(x) = floor(x + 0.5) clamped to
 *   [0, 255] (a NaN gives 0): shade = 0: byte(((q_0 c_0 + q_1 c_1) + q_2 c_2) / s) per channel of the vertices' bytes c;
 *   shade = 1, a HEADLIGHT: the grey byte(255 sh), sh = |n . d| / sqrt((n . n)(d . d)), 0 if sh is not finite, with
 *   n = (Y_1 - Y_0) x (Y_2 - Y_0), d = ((c - cx) / fx, (r - cy) / fy, 1) and every dot product (a_0 b_0 + a_1 b_1) + a_2 b_2.
 *   Empty pixels: index -1, depth and bary NaN, frames (background, background >> 8, background >> 16) & 255
 *   (0 <= background < 2^24).  Every element is written; depth, index and bary may be null.                                  */
#define CPN_RASTER_SMALL 64
#define CPN_RASTER_TILES 256
int cpn_raster_faces(const float* xyz, const int* nvert, const int* faces, const int* nface, const float* poses,
                     const float* intrinsics, int K, int B, int capv, int capf, int H, int W, int cull, double near,
                     unsigned long long* zbuf, void* stream);
int cpn_raster_resolve(const unsigned long long* zbuf, const float* xyz, const uint8_t* rgb, const int* nvert, const int* faces,
                       const float* poses, const float* intrinsics, int K, int B, int capv, int capf, int H, int W, int shade,
                       int background, uint8_t* frames, float* depth, int* index, float* bary, void* stream);

/* ==== the relative pose from the matches alone: 8-point RANSAC (round 20) ================================================
 * cpn_refine_pose is a local method that starts from rel_pose; these three give a pose that depends on the matches only, the
 * inlier count of rel_pose under the same rule, and an inlier mask.  The symbols are additive: the ABI version stays.  The
 * sampler, the solver, the threshold, the scoring and the choice among the four poses are THIS LIBRARY'S definitions.  There is
 * no local optimisation inside the loop (cpn_refine_pose afterwards is that step), no adaptive stopping, no MSAC / MAGSAC
 * scoring (round 24 adds a graded score and the local optimisation, both opt-in); the linear 8-point solver is degenerate for a planar scene and for a pure rotation (round 21 adds the 5-point solver).
 * Conventions: round 16's.  xy (B, N, 4) fp32 = (x0, y0, x1, y1) with count (B) int32 on the device, n = min(max(count, 0), N);
 *   rows at and beyond n are never read.  a = ((x0 - cx0) / fx0, (y0 - cy0) / fy0, 1), b likewise of view 1, float64 from the
 *   fp32 inputs.  X0 = R X1 + t, E = [t]x R, a^T E b = 0; E (.., 9) float64 row-major.  One rounding per operation, sums left to
 *   right, no fused multiply-add.  Hn hypotheses per pair.  1 <= B <= 32767, 1 <= N <= 2^24, Hn <= 2^20 and
 *   B ceil(N / CPN_RANSAC_CHUNK) (Hn + 1) < 2^31 (CPN_E_SHAPE otherwise); inlier_px finite and >= 0 (CPN_E_ARG otherwise).
 * cpn_ransac_hypotheses (Hn >= 1): ONE launch, one thread per (pair, hypothesis index h).
 *   The draw: with mix(z) = splitmix64's finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *   z *= 0x94D049BB133111EB; z ^= z >> 31, 64-bit unsigned) and G = 0x9E3779B97F4A7C15, draw number d = 0, 1, .. of hypothesis h
 *   is u = mix(mix(seed + G (h + 1)) + G (d + 1)) and the row index ((u >> 32) n) >> 32.  The pair index is NOT part of the key:
 *   two equal pairs get equal samples, and a pair's result does not depend on the batch around it.  An index already taken is
 *   skipped and the next draw number is used; after 64 draws without 8 distinct indices (always so for n < 8) the hypothesis
 *   is invalid.  sample (B, Hn, 8) int32: the indices in the order drawn, -1 where none was.
 *   The system: row j of the 8 x 9 matrix is (a0 b0, a0 b1, a0, a1 b0, a1 b1, a1, b0, b1, 1) of sampled match j.
 *   The null vector: Gaussian elimination with COMPLETE pivoting.  Step k = 0 .. 7: the pivot is the entry of the largest
 *   magnitude among rows k .. 7 and columns k .. 8, the first one in (row, column) order on ties; its row and column are
 *   exchanged with row k and column k; RANK TEST: the hypothesis is invalid unless the pivot p_k is finite and
 *   |p_k| > 1e-9 |p_0|; then row r > k becomes row_r - (A_rk / p_k) row_k on the columns beyond k.  Back substitution with
 *   the unknown of the last column set to 1: x_r = -((A_r,r+1 x_r+1 + A_r,r+2 x_r+2) + .. + A_r8 x_8) / A_rr for r = 7 .. 0;
 *   the exchanges of columns are undone; E = x / sqrt((x_0^2 + x_1^2) + .. + x_8^2), negated where its entry of the largest
 *   magnitude (the lower index on ties) is negative.  A hypothesis is invalid also where one of the four values of a sampled row
 *   or a value of E is not finite.  E (B, Hn, 9) float64, all 0 where invalid; valid (B, Hn) bytes 0 / 1.  Every element of
 *   the three outputs is written.
 * cpn_ransac_score: ONE launch over (tiles of 256 slots, chunks of CPN_RANSAC_CHUNK rows, pairs).  Slot h < Hn is hypothesis
 *   h; slot Hn is rel_pose's own E = [t]x R in round 16's expression (rel_pose may be null: the slot is then 0 and nothing is
 *   read).  A match is an INLIER of a slot iff its round-16 residual r under the slot's E counts and |r| <= inlier_px.  partial
 *   (B, ceil(N / CPN_RANSAC_CHUNK), Hn + 1) int32: the inliers of the slot among the chunk's rows below n; 0 for an invalid
 *   hypothesis and for a chunk at or beyond n.  Every element is written.  Integers: exact in any order, no atomics.  Hn may be
 *   0 (E and valid are then not read).
 * cpn_ransac_finish: ONE launch, one workgroup per pair.  usable = the rows below n with four finite values.  The WINNER is the
 *   valid hypothesis with the largest sum of its partial counts, the lower index on ties.  Its E is split by a cyclic one-sided
 *   Jacobi method on the columns of G = E with V = 1: 8 sweeps of the pairs (0, 1), (0, 2), (1, 2); for a pair (p, q) with
 *   alpha = |G_p|^2, beta = |G_q|^2, gamma = G_p . G_q (each (x + y) + z down the rows), nothing where gamma == 0, otherwise
 *   zeta = (beta - alpha) / (2 gamma), tt = sign(zeta) / (|zeta| + sqrt(1 + zeta zeta)) (sign(0) = 1), c = 1 / sqrt(1 + tt tt),
 *   s = c tt, and columns p, q of G and of V become (c x_p - s x_q, s x_p + c x_q).  The columns are then ordered by descending
 *   norm with the exchanges (0, 1), (1, 2), (0, 1), each made only where the earlier norm is strictly smaller.  From columns 0
 *   and 1 of G: u_1 = G_0 / |G_0|, u_2 = w / |w| with w = G_1 - (u_1 . G_1) u_1, u_3 = u_1 x u_2; v_1, v_2, v_3 the same of V.
 *   R1 = (u_2 v_1^T - u_1 v_2^T) + u_3 v_3^T, R2 = (u_1 v_2^T - u_2 v_1^T) + u_3 v_3^T, t = u_3: both rotations are orthonormal
 *   to 1e-12 with determinant +1 by construction.  THE VOTE: every inlier of the winner, with c = R b (row sums
 *   (R_j0 b_0 + R_j1 b_1) + R_j2), z_0 = (t x c) . (a x c) and z_1 = (t x a) . (a x c) - the depths of the point in views 0
 *   and 1 times |a x c|^2 -, votes for (R, +t) where z_0 > 0 and z_1 > 0 and for (R, -t) where z_0 < 0 and z_1 < 0.  The pose is
 *   the candidate with the most votes, the first of (R1, +t), (R1, -t), (R2, +t), (R2, -t) on ties.
 *   pose (B, 4, 4) fp32 = [R | s t], last row 0 0 0 1, with s = sqrt((t0_0^2 + t0_1^2) + t0_2^2) of rel_pose's translation t0
 *   where rel_pose is given, all twelve entries finite and s finite and > 0, otherwise s = 1 (the residual cannot see the
 *   length).  inlier (B, N) bytes: 1 for the inliers of the winner, 0 elsewhere and at and beyond n; every byte is written.
 *   stats (B, 8) float64: [0] the winner's inliers; [1] usable; [2] the winner's index; [3] the number of valid hypotheses;
 *   [4] the inliers of rel_pose (-1 without one); [5], [6] the angles in degrees between R and rel_pose's rotation and between
 *   the signed t and t0 / |t0|, in cpn_refine_pose's two formulas (0 without a usable rel_pose); [7] the status: 0 ok; 1 no
 *   valid hypothesis, or a split that is not finite: pose and inlier as for status 2, [1] and [4] as for status 0, the rest
 *   0; 2 nothing to do (usable < 8 or Hn == 0): pose is rel_pose's 16 values, or the identity without one, inlier is all 0,
 *   [4] is -1 and the other six are 0.  No atomics: bit-reproducible, and a pair's result does not depend on the batch.    */
#define CPN_RANSAC_CHUNK 256
int cpn_ransac_hypotheses(const float* xy, const int* count, const float* intrinsics, int B, int N, int Hn, long long seed,
                          double* E, int* sample, uint8_t* valid, void* stream);
int cpn_ransac_score(const double* E, const uint8_t* valid, const float* xy, const int* count, const float* intrinsics,
                     const float* rel_pose, int B, int N, int Hn, double inlier_px, int* partial, void* stream);
int cpn_ransac_finish(const double* E, const uint8_t* valid, const int* partial, const float* xy, const int* count,
                      const float* intrinsics, const float* rel_pose, int B, int N, int Hn, double inlier_px, float* pose,
                      uint8_t* inlier, double* stats, void* stream);

/* ==== the 5-point solver for round 20's RANSAC: minimal samples (round 21) ================================================
 * The linear 8-point solver is degenerate where the matches lie on one plane; the 5-point solver is not.  One additive symbol:
 * the ABI version stays.  It fills the hypothesis buffers that cpn_ransac_score and cpn_ransac_finish take, with 10 SLOTS per
 * sample: call those two unchanged with Hn' = 10 Hn, E (B, 10 Hn, 9) and valid (B, 10 Hn); slot 10 h + r is root r of sample h,
 * stats [2] is then the winning slot (its sample is stats [2] / 10 rounded down) and stats [3] the number of valid slots.
 * Status 2 of cpn_ransac_finish stays "usable < 8" for both solvers.  Conventions, the draw, the system's rows and the norm and
 * sign of E: round 20's.  1 <= B <= 32767, 1 <= N <= 2^24, 1 <= 10 Hn <= 2^20 and B ceil(N / CPN_RANSAC_CHUNK) (10 Hn + 1) <
 * 2^31 (CPN_E_SHAPE otherwise).  A planar scene has a two-fold ambiguity that only the depth vote of cpn_ransac_finish breaks;
 * a pure rotation gives E = 0 for any solver.  THIS LIBRARY'S definitions, all float64, one rounding per operation, only
 * + - * / sqrt and comparisons, every trip count fixed:
 * cpn_ransac_hypotheses5: ONE launch, one thread per (pair, sample index h).
 *   The draw is round 20's stopped at 5 distinct rows: for equal (seed, h, n) they are the first 5 of cpn_ransac_hypotheses'
 *   8.  The sample is invalid after 64 draws without 5 distinct indices (always so for n < 5) and where one of the four values
 *   of a sampled row is not finite.  sample (B, Hn, 5) int32: the indices in the order drawn, -1 where none was.
 *   The null space: the 5 x 9 system of round 20's rows, round 20's elimination with complete pivoting for steps k = 0 .. 4
 *   (rows k .. 4, columns k .. 8) with its RANK TEST |p_k| > 1e-9 |p_0|.  For v = 0 .. 3 the unknown of permuted column 5 + v
 *   is 1, the other three of columns 5 .. 8 are 0, and x_r = -((A_r,r+1 x_r+1 + A_r,r+2 x_r+2) + .. + A_r8 x_8) / A_rr for
 *   r = 4 .. 0; with the exchanges of columns undone these are X, Y, Z, W (v = 0, 1, 2, 3).  E = x X + y Y + z Z + W.
 *   Polynomials: a linear form is its 4 coefficients of (x, y, z, 1) = variables 0 .. 3; a quadratic its 10 coefficients of the
 *   pairs i <= j, a cubic its 20 of the triples.  lin * lin: every coefficient starts at 0 and takes + a_i b_j for i = 0 .. 3
 *   (outer), j = 0 .. 3 (inner) at the pair {i, j}.  quad * lin: from 0, + a_m b_k for m = the pairs in lexicographic order
 *   (00, 01, 02, 03, 11, 12, 13, 22, 23, 33; outer), k = 0 .. 3 (inner) at the triple.  Sums of polynomials are coefficient-wise.
 *   The constraints, a 10 x 20 matrix M with the columns
 *     x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1:
 *   row 0 is det E = (q0 E_0 - q1 E_1) + q2 E_2 with q0 = E_4 E_8 - E_5 E_7, q1 = E_3 E_8 - E_5 E_6, q2 = E_3 E_7 - E_4 E_6
 *   (entries of E row-major); with G_ij = (E_3i E_3j + E_3i+1 E_3j+1) + E_3i+2 E_3j+2 (i <= j, G symmetric),
 *   half = 0.5 ((G_00 + G_11) + G_22) and L = G with half subtracted from its three diagonal entries, row 1 + 3 i + j is entry
 *   (i, j) of E E^T E - tr(E E^T) E / 2: (L_i0 E_j + L_i1 E_3+j) + L_i2 E_6+j.
 *   Gauss-Jordan elimination, step k = 0 .. 9: the pivot is the entry of the largest magnitude of column k in rows k .. 9, the
 *   first on ties; its row is exchanged with row k; RANK TEST: the sample is invalid unless p_k is finite and
 *   |p_k| > 1e-10 |p_0|; row k is divided by p_k on the columns beyond k; then every row r > k, and every row r with
 *   4 <= r < k, becomes row_r - M_rk row_k on the columns beyond k (rows 0 .. 3 are never read again and are not reduced
 *   upwards).  Rows 4 .. 9 then state x^2z, x^2, y^2z, y^2, xyz, xy by the last ten columns.
 *   B(z): for i = 0, 1, 2 with a = row 4 + 2 i, b = row 5 + 2 i, a - z b = x B_i0(z) + y B_i1(z) + B_i2(z), ascending in z:
 *   B_i0 = (a_12, a_11 - b_12, a_10 - b_11, -b_10), B_i1 = (a_15, a_14 - b_15, a_13 - b_14, -b_13),
 *   B_i2 = (a_19, a_18 - b_19, a_17 - b_18, a_16 - b_17, -b_16).  A product of polynomials in z: from 0, + a_i b_j at i + j, i
 *   outer, j inner.  p1 = B_01 B_12 - B_11 B_02, p2 = B_10 B_02 - B_00 B_12, p3 = B_00 B_11 - B_10 B_01 (the factors in this
 *   order), f = (p1 B_20 + p2 B_21) + p3 B_22, of degree 10.
 *   The Sturm chain: f_0 = f / |f's coefficient 10|; f_1 = f_0' (coefficient k - 1 is k f_0,k); for i = 1 .. 9, with n the
 *   degree of f_(i-1): r = f_(i-1); q = r_n / g with g the leading coefficient of f_i, r_(k+1) -= q f_i,k for k = 0 .. n - 2;
 *   q = r_(n-1) / g, r_k -= q f_i,k for k = 0 .. n - 2; f_(i+1),k = -(r_k / |r_(n-2)|) for k = 0 .. n - 2.  The sample is
 *   invalid where |f's coefficient 10| or an |r_(n-2)| is 0 or not finite.  A polynomial's value is Horner's: v = c_d, then
 *   v = v z + c_k for k = d - 1 .. 0.  V(z) is the number of sign changes of f_0(z) .. f_10(z), zeros skipped; V(-inf) and
 *   V(+inf) are those of the leading coefficients, negated for odd i at -inf.  The number of real roots is
 *   min(max(V(-inf) - V(+inf), 0), 10).
 *   The roots: the real line is z(t) = t / (1 - |t|) for t in (-1, 1).  Root r = 0, 1, .. is found by 40 halvings from
 *   (lo, hi) = (-1, 1): mid = (lo + hi) 0.5; hi = mid where V(-inf) - V(z(mid)) >= r + 1, otherwise lo = mid.  Then
 *   z = z((lo + hi) 0.5) and 4 Newton steps z' = z - f_0(z) / f_1(z), each taken only where z(lo) <= z' <= z(hi).
 *   x = p1(z) / p3(z), y = p2(z) / p3(z), E = ((x X + y Y) + z Z) + W entry by entry, normalised and signed as in round 20.
 *   Slot r of the sample is valid iff the sample is valid, r is below the number of real roots and all nine values of E are
 *   finite; the roots ascend with r.  E (B, Hn, 10, 9) float64, all 0 where invalid; valid (B, Hn, 10) bytes 0 / 1.  Every
 *   element of the three outputs is written.  No atomics: bit-reproducible, and a pair's result does not depend on the batch. */
int cpn_ransac_hypotheses5(const float* xy, const int* count, const float* intrinsics, int B, int N, int Hn, long long seed,
                           double* E, int* sample, uint8_t* valid, void* stream);

/* ==== the homography model for round 20's RANSAC: walls and pure rotations (round 22) ======================================
 * Where one plane or a pure rotation explains the matches the essential matrix is under-determined; the model of that case is
 * a homography.  Three additive symbols: the ABI version stays.  The same three-launch shape as round 20, no atomics, nothing read
 * on the host, bit-reproducible, and a pair's result does not depend on the batch.  Conventions, the draw, the elimination, the
 * one-sided Jacobi method and the shape limits: round 20's (1 <= B <= 32767, 1 <= N <= 2^24, Hn <= 2^20 and
 * B ceil(N / CPN_RANSAC_CHUNK) (Hn + 1) < 2^31, CPN_E_SHAPE otherwise; inlier_px and min_baseline finite and >= 0, CPN_E_ARG
 * otherwise).  a ~ H b, with H = R + t n^T / d for the plane n . X1 = d in view 1's frame; H (.., 9) float64 row-major.  THE
 * TRANSFER-ERROR INLIER RULE, THE VISIBILITY VOTE, THE PICK ORDER AND min_baseline ARE THIS LIBRARY'S definitions; none of them has
 * been tried on a trained checkpoint.  All float64, one rounding per operation, only + - * / sqrt and comparisons.
 * adj(M), the adjugate, row-major: (M4 M8 - M5 M7, M2 M7 - M1 M8, M1 M5 - M2 M4, M5 M6 - M3 M8, M0 M8 - M2 M6, M2 M3 - M0 M5,
 *   M3 M7 - M4 M6, M1 M6 - M0 M7, M0 M4 - M1 M3); det M = (M0 adj0 + M1 adj3) + M2 adj6.  M p for a point p = (p0, p1, 1):
 *   component i is (M_i0 p0 + M_i1 p1) + M_i2.
 * THE INLIER RULE: with m = H b and w = adj(H) a, a match is an inlier of H iff m_2 > 0, m_2 is finite,
 *   d0 = sqrt(dx dx + dy dy) with dx = fx0 (m_0 / m_2 - a0), dy = fy0 (m_1 / m_2 - a1) is finite and d0 <= inlier_px, and the
 *   same holds for w against b in view 1's pixels (w_2 > 0 and finite, fx1 (w_0 / w_2 - b0), fy1 (w_1 / w_2 - b1)).
 * cpn_ransac_homographies (Hn >= 1): ONE launch, one thread per (pair, hypothesis index h).
 *   The draw is round 20's stopped at 4 distinct rows: for equal (seed, h, n) they are the first 4 of cpn_ransac_hypotheses' 8.
 *   The hypothesis is invalid after 64 draws without 4 distinct indices (always so for n < 4) and where one of the four values
 *   of a sampled row is not finite.  sample (B, Hn, 4) int32: the indices in the order drawn, -1 where none was.
 *   The system: sampled match j gives rows 2 j = (b0, b1, 1, 0, 0, 0, -(a0 b0), -(a0 b1), -a0) and
 *   2 j + 1 = (0, 0, 0, b0, b1, 1, -(a1 b0), -(a1 b1), -a1) of an 8 x 9 matrix.  Its null vector x: round 20's elimination with
 *   complete pivoting, its RANK TEST |p_k| > 1e-9 |p_0| (three collinear points and repeated matches fail it) and its back
 *   substitution.  H = x / sqrt((x_0^2 + x_1^2) + .. + x_8^2), negated where det H < 0.  The hypothesis is invalid also where
 *   det H is not finite or not > 0, where a value of H is not finite, and where one of its own four matches has (H b)_2 <= 0 or
 *   (adj(H) a)_2 <= 0: such a homography maps its own sample behind a camera.  H (B, Hn, 9) float64, all 0 where invalid; valid
 *   (B, Hn) bytes 0 / 1.  Every element of the three outputs is written.
 * cpn_ransac_score_h: ONE launch, cpn_ransac_score's grid and tiling over Hn slots (there is no slot for rel_pose: a pose has no
 *   homography without a plane).  partial (B, ceil(N / CPN_RANSAC_CHUNK), Hn) int32: the inliers of hypothesis h among the
 *   chunk's rows below n; 0 for an invalid hypothesis and for a chunk at or beyond n.  Every element is written.  Hn may be 0
 *   (nothing is launched, H, valid and partial are not read).
 * cpn_ransac_finish_h: ONE launch, one workgroup per pair.  usable and the WINNER as in cpn_ransac_finish.  Round 20's Jacobi
 *   method on G = H with V = 1 and its ordering give the column norms sg_0 >= sg_1 >= sg_2; its frames give u_1, u_2, u_3 from G
 *   and v_1, v_2, v_3 = v_1 x v_2 from V.  s1 = sg_0 / sg_1, s3 = sg_2 / sg_1, Hs = H / sg_1 entry by entry.
 *   ROTATION ONLY where s1 s1 - s3 s3 is not > 0 or s1 - s3 <= min_baseline: the pose is [R_n | 0] with
 *   R_n = (u_1 v_1^T + u_2 v_2^T) + u_3 v_3^T, the rotation nearest to H; twin = pose; status 3.  s1 - s3 is the baseline over
 *   the plane's distance, |T| below; where to set min_baseline for real data is unknown, and 0 means "only an exact rotation".
 *   Otherwise THE FOUR CANDIDATES (Ma, Soatto, Kosecka, Sastry, section 5.3): x1 = sqrt(max(1 - s3 s3, 0)),
 *   x3 = sqrt(max(s1 s1 - 1, 0)), den = sqrt(s1 s1 - s3 s3); for k = 0, 1: u = (x1 v_1 + x3 v_3) / den (k = 0) or
 *   (x1 v_1 - x3 v_3) / den (k = 1) component by component; N = v_2 x u; p = Hs v_2, q = Hs u (row sums
 *   (Hs_i0 x_0 + Hs_i1 x_1) + Hs_i2 x_2), r = p x q; R_ij = (p_i v_2j + q_i u_j) + r_i N_j;
 *   T_i = ((Hs_i0 - R_i0) N_0 + (Hs_i1 - R_i1) N_1) + (Hs_i2 - R_i2) N_2; Hs = R + T N^T.  Candidate 2 k is (R, T, N), candidate
 *   2 k + 1 is (R, -T, -N).  E_k = [T]x R in round 16's expression.
 *   THE VOTE: every inlier of the winner (under H as it was scored), with nb = (N_0 b0 + N_1 b1) + N_2, votes for candidate 2 k
 *   where nb > 0 and for 2 k + 1 where nb < 0: the plane must lie in front of camera 1.  samp_k = the rows below n that are
 *   inliers of E_k under cpn_ransac_score's rule with the same inlier_px.  THE PICK: the candidate with the most votes; on a tie
 *   the one with the larger samp_k; on a tie the lower index.  THE TWIN: of the other k, the candidate with more votes, the even
 *   one on a tie.  A fronto-parallel plane in a narrow field of view can leave the vote tied: stats [4] = [5] and [6] = [7] then
 *   say that the ambiguity was not resolved.
 *   pose, twin (B, 4, 4) fp32 = [R | s (+-T / |T|)], |T| = sqrt((T_0^2 + T_1^2) + T_2^2), s as in cpn_ransac_finish (rel_pose is
 *   only measured against).  Hout (B, 9) float64 = Hs (sigma_2 = 1, det > 0).  inlier (B, N) bytes: the inliers of the winner,
 *   0 elsewhere and at and beyond n; every byte is written.  stats (B, 12) float64: [0] the winner's inliers; [1] usable; [2] the
 *   winner's index; [3] valid hypotheses; [4] votes of the pose; [5] votes of the twin; [6] samp of the pose; [7] samp of the
 *   twin; [8] s1; [9] s3; [10] s1 - s3; [11] the status: 0 ok; 1 no valid hypothesis or a decomposition that is not finite: pose
 *   and twin are rel_pose's 16 values, or the identity without one, Hout and inlier 0, [1] usable, the rest 0; 2 nothing to do
 *   (usable < 4 or Hn == 0): as status 1 with [1] = 0; 3 rotation only: [0] .. [3] and [8] .. [10] as for status 0, [4] .. [7] 0. */
int cpn_ransac_homographies(const float* xy, const int* count, const float* intrinsics, int B, int N, int Hn, long long seed,
                            double* H, int* sample, uint8_t* valid, void* stream);
int cpn_ransac_score_h(const double* H, const uint8_t* valid, const float* xy, const int* count, const float* intrinsics, int B,
                       int N, int Hn, double inlier_px, int* partial, void* stream);
int cpn_ransac_finish_h(const double* H, const uint8_t* valid, const int* partial, const float* xy, const int* count,
                        const float* intrinsics, const float* rel_pose, int B, int N, int Hn, double inlier_px,
                        double min_baseline, float* pose, float* twin, double* Hout, uint8_t* inlier, double* stats, void* stream);

/* ==== which model explains a pair: the refined homography and GRIC (round 23) ==============================================
 * Rounds 20 - 22 estimate an essential matrix and a homography; this round says which to believe - E, one plane, or a rotation
 * alone - and refines the homography first, because on minimal 4-point winners the verdict is not reliable.  Two additive
 * symbols: the ABI version stays.  One launch each, one workgroup of 256 threads per pair, no atomics, nothing read on the host,
 * bit-reproducible, and a pair's result does not depend on the batch.  Conventions: rounds 16 and 22 (xy (B, N, 4) fp32 =
 * (x0, y0, x1, y1), count (B) int32, n = min(max(count, 0), N), a and b the normalised points of views 0 and 1, a ~ H b,
 * X0 = R X1 + t, intrinsics (B, 2, 4, 4) fp32 with fx, fy, cx, cy at entries 0, 5, 2, 6).  1 <= B <= 32767 and 1 <= N <= 2^24
 * (CPN_E_SHAPE otherwise).  THE RESIDUAL, THE WEIGHTS, THE GAUGE, sigma_px AND ITS DEFAULT, THE TIE RULE AND THE (d, k) TABLE ARE
 * THIS LIBRARY'S definitions; none of them has been tried on a trained checkpoint.  All float64 from the fp32 inputs, one rounding
 * per operation, + - * / sqrt and comparisons (the rotation step alone takes a sine and a cosine, as cpn_refine_pose's does).
 * THE HOMOGRAPHY'S SAMPSON RESIDUAL of a match under H (row-major): m = H b, component i (H_i0 b0 + H_i1 b1) + H_i2;
 *   C0 = m0 - a0 m2, C1 = m1 - a1 m2; the Jacobian of C in the PIXELS (x0, y0, x1, y1): J00 = -m2 / fx0,
 *   J02 = (H00 - a0 H20) / fx1, J03 = (H01 - a0 H21) / fy1, J11 = -m2 / fy0, J12 = (H10 - a1 H20) / fx1,
 *   J13 = (H11 - a1 H21) / fy1, J01 = J10 = 0.  S = J J^T: A = (J00 J00 + J02 J02) + J03 J03, Bq = J02 J12 + J03 J13,
 *   Cq = (J11 J11 + J12 J12) + J13 J13.  l00 = sqrt(A), l10 = Bq / l00, l11 = sqrt(Cq - l10 l10); y0 = C0 / l00,
 *   y1 = (C1 - l10 y0) / l11; e^2 = y0 y0 + y1 y1: to first order the squared distance in pixels from the match to the matches
 *   that satisfy H, the same kind of quantity as the squared round-16 residual r^2 under E.  The residual COUNTS iff A > 0,
 *   Cq - l10 l10 > 0 and m, C, A, Bq, Cq, l, y and e^2 are all finite.
 *   ALONG a direction dH: dm, dC and dJ are the expressions of m, C and J on dH (with a and b as they are);
 *   dA = 2 ((J00 dJ00 + J02 dJ02) + J03 dJ03), dBq = ((dJ02 J12 + J02 dJ12) + dJ03 J13) + J03 dJ13,
 *   dCq = 2 ((J11 dJ11 + J12 dJ12) + J13 dJ13); dl00 = dA / (2 l00), dl10 = (dBq - l10 dl00) / l00,
 *   dl11 = (dCq - (2 l10) dl10) / (2 l11); dy0 = (dC0 - y0 dl00) / l00, dy1 = (((dC1 - dl10 y0) - l10 dy0) - y1 dl11) / l11: the
 *   FULL derivative of y, the whitening differentiated with it.
 * cpn_refine_homography: cpn_refine_pose's robust Gauss-Newton with that residual.  H0 (B, 9) float64; mode 0 the plane, 1 the
 *   rotation alone; iters >= 0; scale_px finite and > 0 (CPN_E_ARG otherwise).
 *   MODE 0: the state is h with |h|_F = 1: H0 / sqrt((H0_0^2 + H0_1^2) + .. + H0_8^2), negated where its determinant (round 22's
 *   expression) is < 0; the sign is not looked at again.  The nine directions are the unit matrices, parameter k = entry k.
 *   MODE 1: the state is the rotation nearest to H0, R_n = (u_1 v_1^T + u_2 v_2^T) + u_3 v_3^T from round 20's Jacobi method and
 *   frames on G = H0, exactly as cpn_ransac_finish_h forms it for status 3; H = R; the three directions are [e_k]x R.
 *   A PASS: thread t adds the rows t, t + 256, .. below n in ascending order, the 64 lanes of a wave by the xor butterfly
 *   32 .. 1, the four waves as (0 + 1) + (2 + 3).  A row whose residual counts has u = 1 + e^2 / (scale_px scale_px),
 *   w = 1 / (u u) and, with J0_k = dy0 and J1_k = dy1 along direction k, adds (w J0_j) J0_k + (w J1_j) J1_k to entry (j, k >= j)
 *   of the normal matrix, (w J0_j) y0 + (w J1_j) y1 to entry j of the gradient, (e^2 / 2) / u to the cost, w to the weights and 1
 *   to the rows.  THE STEP: A_jj += 1e-3 A_jj; in mode 0 then A += (tr / 9) h h^T with tr the trace before the damping, the
 *   gauge (the residual cannot see the length of h: cpn_refine_pose's translation gauge at nine parameters); delta = -A^-1 g
 *   by Cholesky as in cpn_refine_pose; mode 0: h <- (h + delta) / |h + delta|; mode 1: R <- exp([delta]x) R by cpn_refine_pose's
 *   Rodrigues step.  A pivot that is not > 0 or a value that is not finite keeps the state, sets status 1 and ends the pair's
 *   passes.  Pass `iters` only measures.
 *   H (B, 9) float64: the unit h (mode 0) or the rotation (mode 1).  pose (B, 4, 4) fp32: [R | 0] above 0 0 0 1 in mode 1, the
 *   identity in mode 0.  stats (B, 8) float64: [0] the cost of pass 0; [1], [2], [3] the cost, the sum of weights and the rows
 *   that count at the returned state; [4] how far the state moved: |h - h_start|_F in mode 0, the angle in degrees in
 *   cpn_refine_pose's formula in mode 1; [5] sigma_1 - sigma_3 of the returned H over sigma_2 (the column norms of round 20's
 *   Jacobi method) in mode 0, 0 in mode 1; [6] the updates made; [7] the status: 0 ok; 1 a failed solve; 2 nothing to do (n == 0,
 *   iters == 0, an H0 that is all zero or not finite, a start that is not finite): H is H0's nine values, pose the identity,
 *   the other stats 0.  Every element of the three outputs is written.
 * cpn_model_gric: Torr's GRIC with r = 4 and lambda = (ln 4, ln 4n, 2) over three models.  pose_e (B, 4, 4) fp32, its
 *   E = [t]x R in round 16's expression; H_plane, H_rot (B, 9) float64; avail (B, 3) bytes: whether model m takes part;
 *   sigma_px finite and > 0 (CPN_E_ARG otherwise); ln4n (N + 1) float64, entry u = ln(4 u) AS THE CALLER COMPUTED IT ON THE
 *   HOST (entry 0 is not read): the kernel takes no logarithm, and ln 4 is the constant 1.3862943611198906.
 *   USABLE rows: below n with four finite values; n_u their number.  Model m = 0, 1, 2 (E, plane, rotation) has
 *   (d, k) = (3, 5), (2, 8), (2, 3) and cap_m = 2 (4 - d_m).  It is IN iff avail is not 0 and its nine values are finite.
 *   x = e^2 / (sigma_px sigma_px) with e^2 = r r for E (r = n / sqrt(D), round 16) and the residual above for the other two.  A
 *   usable row is BELOW THE CAP of a model that is in iff its residual counts and x < cap_m; rho = x there and cap_m otherwise.
 *   gric_m = (sum rho + (ln 4 d_m) n_u) + ln4n[n_u] k_m, the sum in the order of a pass above; +inf where the model is out or
 *   n_u = 0.  THE PICK: the smallest gric; a tie goes to the model with fewer parameters: rotation, then plane, then E.
 *   gric (B, 3) float64.  label (B, N) bytes: bit m set iff the row is usable and below the cap of model m; 0 elsewhere and at
 *   and beyond n; every byte is written.  stats (B, 7) float64: [0] the pick, -1 where no model is in; [1] n_u; [2], [3], [4]
 *   the rows below the cap per model (0 for a model that is out); [5] the runner-up's gric minus the winner's, +inf with fewer
 *   than two models in; [6] the status: 0 ok; 1 no model in; 2 n_u = 0.  sigma_px = 0.5, the wrapper's default, is half the
 *   default inlier_px and as untried on a trained checkpoint as that is.                                                      */
int cpn_refine_homography(const float* xy, const int* count, const float* intrinsics, const double* H0, int B, int N, int mode,
                          int iters, double scale_px, double* H, float* pose, double* stats, void* stream);
int cpn_model_gric(const float* xy, const int* count, const float* intrinsics, const float* pose_e, const double* H_plane,
                   const double* H_rot, const uint8_t* avail, const double* ln4n, int B, int N, double sigma_px, double* gric,
                   uint8_t* label, double* stats, void* stream);

/* ==== LO-MSAC for round 20's RANSAC: a graded integer score and local optimisation inside the loop (round 24) ==============
 * Round 20's loop scores a hypothesis by a bare inlier count and refines only the one that wins.  Three additive symbols - the ABI
 * version stays - give it a graded score and let the K best-scoring hypotheses be polished BEFORE the winner is chosen, on the
 * device: a fixed number of launches, no atomics, nothing read on the host, bit-reproducible, a pair's result independent of the
 * batch.  Both parts are opt-in: cpn_ransac_score and cpn_ransac_finish are what they were.  Both solvers (rounds 20 and 21) fill
 * the hypothesis buffers; Hn below is the number of SLOTS (10 per sample for the 5-point solver).  Conventions, the residual, the
 * inlier rule, the split, the vote, the norm and sign of E: round 20's.  THE 2^20 FIXED POINT, K, THE NUMBER OF PASSES, THE
 * SCALE OF THE WEIGHTS AND THE RANK AND TIE RULES ARE THIS LIBRARY'S definitions; none of them has been tried on a trained
 * checkpoint.  Shapes: 1 <= B <= 32767, 1 <= N <= 2^24, 0 <= K <= CPN_RANSAC_LO_MAX, Hn + K <= 2^20 and
 * B ceil(N / CPN_RANSAC_CHUNK) (Hn + K + 1) < 2^31 (CPN_E_SHAPE otherwise); inlier_px finite and >= 0, graded 0 or 1, iters >= 0,
 * scale_px finite and > 0 (CPN_E_ARG otherwise).
 * THE GRADED SCORE: the WEIGHT of a match under a slot's E is 0 where the match is no inlier of the slot (round 20's rule) and
 *   otherwise floor(CPN_MSAC_ONE (1 - (r r) / (inlier_px inlier_px))) in float64, held to [0, CPN_MSAC_ONE], with r the round-16
 *   residual; CPN_MSAC_ONE where inlier_px == 0; 0 where the quotient is not a number.  A slot's score is the sum of its weights:
 *   an integer in units of 2^-20 inlier, at most 2^28 over a chunk (an int32 partial) and 2^44 over a pair (summed in int64).
 * cpn_ransac_score_slots: cpn_ransac_score's launch on a RANGE of a wider row.  E (B, Hn, 9) and valid (B, Hn) are scored into
 *   columns first .. first + Hn - 1 of partial (B, ceil(N / CPN_RANSAC_CHUNK), total + 1) int32, first + Hn <= total; the call
 *   with first + Hn == total also scores rel_pose's own E into column `total` (0 there without rel_pose).  graded 0: the inlier
 *   counts of cpn_ransac_score; 1: the sums of weights.  The other columns are not touched; a call with nothing to score launches
 *   nothing.
 * cpn_ransac_polish (K >= 1): ONE launch, grid (K, B), one workgroup per (rank k, pair).  partial (B, chunks, Hn + K + 1) holds
 *   the scores of the Hn hypotheses in its first Hn columns.  THE RANK: the order of the valid hypotheses is (score descending,
 *   slot ascending) with the score the int64 sum of the slot's partials below n; rank k is the k-th of that order from 0.
 *   Where usable < 8 (round 20's count) or there are no more than k valid hypotheses, polished slot k is INVALID: E_lo 0,
 *   valid_lo 0, info (-1, -1, 0, 0, 0, 0, 0, 2).  Otherwise the slot's E is split and its inliers under inlier_px vote exactly as
 *   in cpn_ransac_finish (a split that is not finite: invalid with info [7] = 3 and [0], [1] = -1); the picked candidate (R, +-t)
 *   is the start of cpn_refine_pose's passes - the same sums in the same order, the same damping, gauge, Cholesky solve and
 *   Rodrigues step - over ALL rows below n with weights 1 / (1 + (r / scale_px)^2)^2: `iters` updates, ended early by a failed
 *   solve, which keeps the state before it.  E_lo (B, K, 9) float64 = [t]x R of the final state in round 16's expression,
 *   normalised and signed as cpn_ransac_hypotheses' E; valid_lo (B, K) bytes; info (B, K, 8) float64: [0] the slot polished,
 *   [1] its rank k, [2] the updates made, [3 - 6] the four vote counts, [7] 0 ok, 1 a failed solve (the slot is valid all the
 *   same), 2, 3 as above (3 also where E_lo is not finite).  Every element of the three outputs is written.
 * cpn_ransac_finish_lo: cpn_ransac_finish over Hn + K slots, slot Hn + k the polished slot k, partial (B, chunks, Hn + K + 1)
 *   with rel_pose's column last.  The winner is the valid slot with the largest int64 sum, the LOWER slot on ties: a polished
 *   slot wins only where it scores strictly higher, so the winning score never falls below that of the hypotheses alone.  graded
 *   says which score partial holds.  pose, inlier and stats as cpn_ransac_finish's: [0] stays the winner's INLIERS and [4] those
 *   of rel_pose - with graded 1 both are counted in the pass that writes `inlier` -, [2] is the winning slot (>= Hn: a polished
 *   one), [3] counts the valid ones among all Hn + K.  score (B) int64: the winner's score, 0 where the status is not 0.  lo
 *   (B, 4) float64: [0] 1 where a polished slot won, else 0; [1] the slot it was polished from, [2] that slot's rank (both -1
 *   where none won); [3] the updates made (0 where none won).  K may be 0 (E_lo, valid_lo and info are then not read).      */
#define CPN_MSAC_ONE 1048576
#define CPN_RANSAC_LO_MAX 16
int cpn_ransac_score_slots(const double* E, const uint8_t* valid, const float* xy, const int* count, const float* intrinsics,
                           const float* rel_pose, int B, int N, int Hn, int first, int total, int graded, double inlier_px,
                           int* partial, void* stream);
int cpn_ransac_polish(const double* E, const uint8_t* valid, const int* partial, const float* xy, const int* count,
                      const float* intrinsics, int B, int N, int Hn, int K, int iters, double inlier_px, double scale_px,
                      double* E_lo, uint8_t* valid_lo, double* info, void* stream);
int cpn_ransac_finish_lo(const double* E, const uint8_t* valid, const double* E_lo, const uint8_t* valid_lo, const double* info,
                         const int* partial, const float* xy, const int* count, const float* intrinsics, const float* rel_pose,
                         int B, int N, int Hn, int K, int graded, double inlier_px, float* pose, uint8_t* inlier, double* stats,
                         long long* score, double* lo, void* stream);

/* ==== how good is a pose, and how good are the matches under it: float64 pose errors and exact residual quantiles (round 25) ===
 * Rounds 16 and 20 - 24 estimate poses; this round measures them against a ground truth, on the device, for Evaluator's table.  Two
 * additive symbols: the ABI version stays.  One launch each, no atomics in global memory, no device value read on the host,
 * bit-reproducible, and a (pair, pose)'s result does not depend on the batch.  Conventions: round 16's (xy (B, N, 4) fp32 =
 * (x0, y0, x1, y1), count (B) int32, n = min(max(count, 0), N), rows at and beyond n are never read, intrinsics (B, 2, 4, 4) fp32
 * with fx, fy, cx, cy at entries 0, 5, 2, 6, a pose row-major [R | t] with X0 = R X1 + t).  1 <= B <= 32767, 1 <= N <= 2^24 and
 * 1 <= P, Q, T <= CPN_POSE_EVAL_MAX (CPN_E_SHAPE otherwise).  THE RANK RULE, THE LMedS FACTOR WITH p = 5, THE 2.5 SIGMA CUT AND THE
 * ANGLE FORMULA ARE THIS LIBRARY'S definitions; none of them has been tried on a trained checkpoint.  All float64 from the fp32
 * inputs, one rounding per operation, sums left to right as the parentheses say; |v| of three values is
 * sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2).
 * cpn_pose_errors: one thread per (pair, pose).  poses (B, P, 4, 4) fp32, gt (B, 4, 4) fp32, out (B, P, 3) float64, in the
 *   reference's units (radians and scene units).  M = R R_gt^T, M_ij = (R_i0 G_j0 + R_i1 G_j1) + R_i2 G_j2.
 *   [0] the rotation angle atan2(0.5 |(M21 - M12, M02 - M20, M10 - M01)|, (((M00 + M11) + M22) - 1) / 2): the sine from the
 *   antisymmetric part and the cosine from the trace, so that the angle is well conditioned at 0 and at pi, where acos of the
 *   cosine alone is not;  [1] the translation distance |t - t_gt|;  [2] the direction angle atan2(|t x t_gt|, t . t_gt) with
 *   t x g = (t_1 g_2 - t_2 g_1, t_2 g_0 - t_0 g_2, t_0 g_1 - t_1 g_0) and t . g = (t_0 g_0 + t_1 g_1) + t_2 g_2; NaN where t or
 *   t_gt is (0, 0, 0).  Where one of the twelve values of the pose or of gt is not finite all three are NaN, in that entry alone.
 *   atan2 is the device library's; the other operations are exact to the last bit.
 * cpn_residual_stats: grid (P, B), one workgroup of 256 threads per (pose, pair), cpn_refine_pose's shape.  poses (B, P, 4, 4)
 *   fp32; q (Q) float64, each in [0, 1], and thr (T) float64, each finite and >= 0 (CPN_E_ARG otherwise): HOST arrays, checked
 *   here and handed to the kernel as arguments - 16 doubles, no copy, and a bad value is a status code.  The residual of a row is
 *   round 16's r = n / sqrt(D) under E = [t]x R of the pose as it comes (t is not normalised); the row is USABLE iff the
 *   residual counts (round 16's rule); its key is |r|, so -0 and +0 are one value.
 *   usable (B, P) int32 = n_u.  quant (B, P, Q) float64 = the element of rank floor(q (n_u - 1)) - the product in float64 - of
 *   the usable |r| in ascending order: no interpolation, every value is one of the residuals in its bits, and q = 0.5 is the
 *   lower middle.  within (B, P, T) int32 = the usable rows with |r| <= thr.  sigma (B, P, 2) float64: with med the element of
 *   rank (n_u - 1) / 2 rounded down, [0] = (1.4826 (1 + 5 / (n_u - 5))) med, Rousseeuw's LMedS scale for p = 5 parameters, NaN for
 *   n_u <= 5; [1] = sqrt(S / (n_in - 5)) with n_in the usable rows with |r| <= 2.5 [0] and S the sum of their r r in the order of
 *   a pass of cpn_refine_pose (thread t adds the rows t, t + 256, .. in ascending order from 0, the 64 lanes of a wave by the xor
 *   butterfly 32 .. 1, the four waves as (0 + 1) + (2 + 3)), NaN for n_in <= 5.  status (B, P) int32: 0 ok; 1 no usable row; 2 a
 *   pose with a value that is not finite or with t = (0, 0, 0); for 1 and 2 usable and within are 0 and quant and sigma NaN.
 *   Every element of the five outputs is written.
 *   THE SELECTION is a radix descent on the 64-bit pattern of |r| (non-negative doubles order as their patterns), 8 bits a pass
 *   from the top, with the residual recomputed in every pass from the same inputs and the digit counts kept in LDS as integers:
 *   ten passes over the rows below n, no sort, no scratch in global memory.  N = 131 072 rows and more work.                     */
#define CPN_POSE_EVAL_MAX 8
int cpn_pose_errors(const float* poses, const float* gt, int B, int P, double* out, void* stream);
int cpn_residual_stats(const float* xy, const int* count, const float* intrinsics, const float* poses, const double* q,
                       const double* thr, int B, int N, int P, int Q, int T, int* usable, double* quant, int* within, double* sigma,
                       int* status, void* stream);

/* ==== the matches as geometry: optimal two-view triangulation and the length of the baseline (round 26) ========================
 * Rounds 16 and 20 - 25 stop at the pose.  This round turns the matches into 3-D points under a pose and, against a depth map of
 * view 0, into the one number the epipolar residual cannot see: the translation's length.  Two additive symbols: the ABI version
 * stays.  One launch each, no atomics in global memory, no device value read on the host, bit-reproducible, and a row's (a
 * pair's) result does not depend on the batch.  Conventions: round 16's (xy (B, N, 4) fp32 = (x0, y0, x1, y1) = (x, x'), count (B)
 * int32, n = min(max(count, 0), N), intrinsics (B, 2, 4, 4) fp32 with fx, fy, cx, cy at entries 0, 5, 2, 6, a pose row-major
 * [R | t] with X0 = R X1 + t, a of view 0, b of view 1, a^T E b = 0).  1 <= B <= 32767, 1 <= N <= 2^24 (CPN_E_SHAPE otherwise).
 * THE PASS COUNT, THE FLAG RULES, THE KEEP RULE AND ITS DEFAULTS, THE NEAREST-PIXEL READ AND THE MEDIAN RULE ARE THIS LIBRARY'S
 * definitions; none of them has been tried on a trained checkpoint.  All float64 from the fp32 inputs, one rounding per operation,
 * sums left to right as the parentheses say; |v| of three values is sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2), u x v =
 * (u_1 v_2 - u_2 v_1, u_2 v_0 - u_0 v_2, u_0 v_1 - u_1 v_0), u . v = (u_0 v_0 + u_1 v_1) + u_2 v_2.
 * cpn_triangulate_matches: one thread per (pair, row).  pose (B, 4, 4) fp32; images NULL, or (B, 2, S, S, 3) fp32 in [-1, 1] (the
 *   pair's two photos, `context.rgb`), 1 <= S <= 16384; rgb may be NULL iff images is.  Outputs xyz (B, N, 3) fp32, geom (B, N, 4)
 *   fp32, flag (B, N) uint8, rgb (B, N, 3) fp32; every element is written.  Rows at and beyond n: NaN and flag 255.  A row with a
 *   value that is not finite, and every row of a pair whose pose or intrinsics hold a value that is not finite or whose t is
 *   (0, 0, 0): NaN and flag CPN_TRI_INPUT alone.  Every other row:
 *   THE CORRECTION (Lindstrom's rule in the iterated form; only + - x / sqrt, CPN_TRIANGULATE_PASSES passes).  th = t / |t|,
 *   E = [th]x R (round 16's entries), a = ((x0 - cx0) / fx0, (y0 - cy0) / fy0, 1), b likewise from (x1, y1) and camera 1,
 *   c = a^T E b = round 16's n, n0 = ((E b)_0 / fx0, (E b)_1 / fy0), n0' = ((E^T a)_0 / fx1, (E^T a)_1 / fy1) - round 16's g: with
 *   F = K0^-T E K1^-1 they are x^T F x', (F x')_12 and (F^T x)_12 -, and Ft_ij = (E_ij / f0_i) / f1_j for i, j < 2 with
 *   f0 = (fx0, fy0), f1 = (fx1, fy1): the upper-left 2 x 2 of F.  From n = n0, n' = n0', every pass:
 *     A = n_0 (Ft_00 n'_0 + Ft_01 n'_1) + n_1 (Ft_10 n'_0 + Ft_11 n'_1);   Bq = 0.5 ((n_0 n0_0 + n_1 n0_1) + (n'_0 n0'_0 + n'_1 n0'_1));
 *     disc = Bq Bq - A c;   d = sqrt(disc);   den = Bq + d;   lambda = c / den;   D = lambda n;   D' = lambda n';
 *     n_i = n0_i - (Ft_i0 D'_0 + Ft_i1 D'_1);   n'_j = n0'_j - (Ft_0j D_0 + Ft_1j D_1).
 *   A pass in which disc >= 0 or den != 0 does not hold sets CPN_TRI_CORRECTION (a match on both epipoles does: everything is 0).
 *   The corrected match is xh = x - D, xh' = x' - D' with the last pass's D, D'.  c - 2 Bq lambda + A lambda^2 = 0 in every pass,
 *   so (xh, xh') lies on the constraint after any number of passes; further passes slide it towards the closest such pair.
 *   THE POINT.  ah, bh the normalised xh, xh' (as a, b above); cr_j = (R_j0 bh_0 + R_j1 bh_1) + R_j2;  w = ah x cr;  ww = w . w;
 *   z0 = ((t x cr) . w) / ww;  z1 = ((t x ah) . w) / ww - round 20's two cheirality numerators over ww, with t AS GIVEN: the caller
 *   decides the length -;  X = (z0 ah_0, z0 ah_1, z0), in view 0's frame.  CPN_TRI_PARALLAX unless ww > 0, CPN_TRI_BEHIND0 unless
 *   z0 > 0, CPN_TRI_BEHIND1 unless z1 > 0 (a NaN sets them).
 *   xyz = X; geom = (z0, z1, sqrt(((D_0 D_0 + D_1 D_1) + D'_0 D'_0) + D'_1 D'_1) - the reprojection error in pixels -,
 *   atan2(sqrt(ww), ah . cr) 57.29577951308232 - the parallax in degrees; atan2 is the device library's, every other operation is
 *   exact to the last bit), each rounded to fp32 once.
 *   rgb, per channel: 0.5 (s0 + s1) with s_v the bilinear sample of image v at the match AS GIVEN: u = min(max(x, 0), S - 1),
 *   i = min(floor(u), S - 2) (0 for S = 1), l = u - i, likewise along y, s = (1 - ly) ((1 - lx) p00 + lx p01) + ly ((1 - lx) p10 +
 *   lx p11) with the taps clamped to the image.
 * cpn_depth_scale: grid B, one workgroup of 256 threads per pair.  geom and flag as cpn_triangulate_matches wrote them for a pose
 *   with |t| = 1; depth (B, S S) fp32, a z-depth map of view 0 on the S x S grid; rel_pose NULL or (B, 4, 4) fp32; max_reproj_px
 *   and min_parallax_deg finite and >= 0, min_rows >= 1 (CPN_E_ARG otherwise).  Row i < n is USED iff flag = 0, geom_2 <=
 *   max_reproj_px, geom_3 >= min_parallax_deg, the NEAREST pixel (floor(x0 + 0.5), floor(y0 + 0.5)) lies in the grid, the depth d
 *   read there counts by round 14's rule (finite, 0 < d < 10), and q = d / geom_0 (both converted to float64) is finite and > 0.
 *   scale (B) float64 = the element of rank (n_u - 1) / 2 rounded down of the used q in ascending order - round 25's rank rule:
 *   the LOWER median, one of the q in its bits.  stats (B, 4) float64: [0] n_u; [1] the element of the same rank of
 *   |q / scale - 1|; [2] |t| of rel_pose / scale, NaN without one; [3] 0 ok, 1 n_u < min_rows: scale, [1] and [2] are NaN.
 *   The selection is round 25's radix descent (radix_select.h), twice: sixteen passes over the rows below n.                       */
#define CPN_TRIANGULATE_PASSES 3
#define CPN_TRI_INPUT 1
#define CPN_TRI_CORRECTION 2
#define CPN_TRI_PARALLAX 4
#define CPN_TRI_BEHIND0 8
#define CPN_TRI_BEHIND1 16
int cpn_triangulate_matches(const float* xy, const int* count, const float* intrinsics, const float* pose, const float* images,
                            int B, int N, int S, float* xyz, float* geom, uint8_t* flag, float* rgb, void* stream);
int cpn_depth_scale(const float* geom, const uint8_t* flag, const float* xy, const int* count, const float* depth,
                    const float* rel_pose, int B, int N, int S, double max_reproj_px, double min_parallax_deg, int min_rows,
                    double* scale, double* stats, void* stream);

/* ==== two-view bundle adjustment over the pose and the points, with covariances (round 27) =====================================
 * Round 16's refinement minimises the Sampson residual and round 26 places the points under a pose that something else found.
 * This round minimises the reprojection error itself over the pose and one point per match, by Levenberg-Marquardt on the Schur
 * complement of the points, and states the Gauss-Newton covariance of the pose and of every point.  One additive symbol: the ABI
 * version stays.  One launch, grid B, ONE workgroup of 256 threads per pair, every sweep inside it; no atomics, no device value
 * read on the host, bit-reproducible, and a pair's result does not depend on the batch.  Conventions: round 26's.  THE GAUGE, THE
 * FORMULA OF sigma, THE LM CONSTANTS, THE STOP RULE AND THE USED-ROW RULE ARE THIS LIBRARY'S definitions; the covariance is the
 * Gauss-Newton one (it ignores the weights' derivative and the outliers); none of it has been tried on a trained checkpoint.
 * All float64 from the fp32 inputs, one rounding per operation, sums left to right as the parentheses say; |v|, u x v and u . v as
 * in round 26; "d += l d" stands for d = d + l d.
 * cpn_bundle_adjust: xy, count, intrinsics, pose (B, 4, 4) fp32 as in round 26; xyz_in (B, N, 3) fp32 and flag (B, N) uint8 as
 *   cpn_triangulate_matches wrote them under that pose; inlier NULL or (B, N) uint8; iters >= 0, scale_px and ftol finite, scale_px
 *   > 0, ftol >= 0, min_rows >= 1 (CPN_E_ARG otherwise); 1 <= B <= 32767, 1 <= N <= 2^24 (CPN_E_SHAPE).  work (B, 2, N, 3)
 *   float64 holds the kept and the tentative points: in HBM (L2 for a pair of 6 000 rows: 288 KB), NOT in LDS, so that a pair of
 *   131 072 rows works.  Outputs: pose_out (B, 4, 4) fp32, xyz (B, N, 3) fp32, geom (B, N, 4) fp32, cov_x (B, N, 6) fp32, cov
 *   (B, 6, 6) float64, stats (B, CPN_BUNDLE_STATS) float64; every element is written.
 *   THE STATE.  len0 = |t| of pose, R, th = t / len0, and per row the point X = xyz_in / len0 (each coordinate converted, then
 *   divided), in view 0's frame, X0 = R X1 + th.  R is taken as given and only ever multiplied from the left by exact rotations: it
 *   is NOT re-orthonormalised, and an fp32 pose's R^T R - I (5e-8) stays in pose_out, as in round 16.  Row i < n is USED iff its four coordinates and X are finite, flag_i = 0, inlier_i
 *   != 0 where given, and X_2 > 0 and Y_2 > 0 with Y = R^T (X - th) (below).  A pair is NOT USABLE (status 2) iff pose or the
 *   intrinsics hold a value that is not finite, t = (0, 0, 0) or fewer than min_rows rows are used: pose_out = pose, every other
 *   output NaN but stats[3] = the used rows (0 where the pose is at fault), stats[4] = stats[5] = 0 and stats[11] = 2.
 *   THE RESIDUAL of a used row at (R, th, X):  d = X - th;  Y_j = (R_0j d_0 + R_1j d_1) + R_2j d_2;  r = ((fx0 X_0) / X_2 + cx0 - x0,
 *   (fy0 X_1) / X_2 + cy0 - y0, (fx1 Y_0) / Y_2 + cx1 - x1, (fy1 Y_1) / Y_2 + cy1 - y1);  e2 = ((r_0 r_0 + r_1 r_1) + r_2 r_2) + r_3 r_3;
 *   u = 1 + e2 / (scale_px scale_px);  cost = (e2 / 2) / u;  w = 1 / (u u): round 16's cost and weight.
 *   THE JACOBIANS.  A (2 x 3) = [fx0 / X_2, 0, -((fx0 X_0) / X_2) / X_2; 0, fy0 / X_2, -((fy0 X_1) / X_2) / X_2], P likewise from
 *   camera 1 and Y;  M_ac = (P_a0 R_c0 + P_a1 R_c1) + P_a2 R_c2 (= P R^T);  J_x = [A; M] (4 x 3).  J_p (4 x 6) is 0 in its first two
 *   rows; rows 2 and 3 are [M [d]x, -M]: (M_a1 d_2 - M_a2 d_1, M_a2 d_0 - M_a0 d_2, M_a0 d_1 - M_a1 d_0, -M_a0, -M_a1, -M_a2): the
 *   derivative by round 16's step R <- exp([om]x) R, th <- th + dt, BEFORE th is renormalised - the points are divided by the same
 *   length below, and the residual does not see a common scale.
 *   THE ROW'S BLOCKS, every sum over the residual's rows in ascending order, left to right, w times the column first ((w J_aj) J_ak):
 *   V = w J_x^T J_x (3 x 3, upper triangle mirrored), V_cc += lambda V_cc;  W = w J_p^T J_x (6 x 3; rows 2 and 3 alone);
 *   U = w J_p^T J_p (upper triangle);  gx = w J_x^T r;  gp = w J_p^T r.  Vi = V^-1, column k = round 16's Cholesky solve of
 *   V with the right side -e_k, on a fresh copy of V each;  T = W Vi: T_jc = (W_j0 Vi_0c + W_j1 Vi_1c) + W_j2 Vi_2c.
 *   SWEEP A: thread t walks the used rows t, t + 256, .. in ascending order and adds, where the three solves succeed,
 *   U_jk - ((T_j0 W_k0 + T_j1 W_k1) + T_j2 W_k2) to the 21 sums of S (j <= k, by rows) and gp_j - ((T_j0 gx_0 + T_j1 gx_1) +
 *   T_j2 gx_2) to the 6 of g; and for every used row the cost, w and 1: round 16's 30 sums, reduced as there (wave butterfly 32 .. 1,
 *   then (w0 + w1) + (w2 + w3)).  The KEPT COST is this sweep's cost sum.
 *   THE SOLVE (thread 0): p = ((((S_00 + S_11) + S_22) + S_33) + S_44) + S_55) / 6;  S_jj += lambda S_jj;  the translation block +=
 *   p (th_i th_j);  delta = -S^-1 g by round 16's Cholesky;  R' = exp([delta_012]x) R (Rodrigues, the device library's sin and
 *   cos; the identity below 1e-12), tn = th + delta_345, len = |tn|, th' = tn / len.  A failed solve or a step that is not finite:
 *   status 1, the state is kept and the iteration ends.
 *   SWEEP B: every thread forms V, W, gx and Vi of its rows again at the kept state;  v_c = gx_c + (((((W_0c delta_0 + W_1c delta_1)
 *   + W_2c delta_2) + W_3c delta_3) + W_4c delta_4) + W_5c delta_5);  dX_a = -((Vi_a0 v_0 + Vi_a1 v_1) + Vi_a2 v_2), 0 where the
 *   solves failed;  X' = (X + dX) / len, written to the tentative half of work;  the TRIAL COST is the sum, as in sweep A, of
 *   the cost of X' under (R', th') - or +inf where an X' is not finite or X'_2 > 0 and Y'_2 > 0 do not both hold.
 *   THE CONTROL.  lambda = 1e-3.  Sweep A; then, while fewer than iters solves were made: solve, sweep B;  trial < kept: ACCEPT
 *   (the halves of work and the state change places, lambda = max(lambda / 3, 1e-12); stop if kept - trial <= ftol kept);
 *   otherwise REJECT (lambda = 4 lambda; stop if lambda > 1e8);  sweep A at the kept state with the new lambda.
 *   THE COVARIANCE.  A last sweep A with lambda = 0 gives S0 and stats[1 .. 3];  p = tr S0 / 6 as above, u = (0, 0, 0, th);
 *   Cinv = S0 with its translation block += p (th_i th_j); column k of its inverse by the Cholesky solve with the right side -e_k,
 *   on a fresh copy each;  C_jk = inverse_jk - (u_j u_k) / p: the covariance of (om, dt) in the gauge |th| = 1 for unit pixel
 *   variance.  A failed solve here: cov, cov_x and stats[8], [9] are NaN and the status is 1.  A last sweep, per used row with V, W,
 *   Vi and T at lambda = 0:  CT_jb = sum over k = 0 .. 5, left to right, of C_jk T_kb;  Cov_ab = Vi_ab + (sum over j = 0 .. 5, left to
 *   right, of T_ja CT_jb) for a <= b - NaN where the solves failed.
 *   THE OUTPUTS.  pose_out = [R | len0 th];  xyz = len0 X;  geom = (len0 X_2, len0 Y_2, sqrt(e2), w);  cov_x = (len0 len0) (Cov_00,
 *   Cov_01, Cov_02, Cov_11, Cov_12, Cov_22);  cov = C;  rows that are not used, and rows at and beyond n: NaN.  stats: [0] the cost
 *   of the first sweep A, [1] the last one's cost, [2] its sum of w, [3] the used rows, [4] steps accepted, [5] rejected, [6] the
 *   last lambda, [7] sigma = sqrt((2 cost) / (rows - 5)), NaN at rows <= 5, [8] sigma sqrt((C_00 + C_11) + C_22) 57.29577951308232,
 *   [9] sigma sqrt((C_33 + C_44) + C_55) 57.29577951308232, [10] round 16's angle in degrees from pose's rotation to R, [11] the
 *   status: 0 ok, 1 a solve failed, 2 not usable.                                                                                  */
#define CPN_BUNDLE_STATS 12
int cpn_bundle_adjust(const float* xy, const int* count, const float* intrinsics, const float* pose, const float* xyz_in,
                      const uint8_t* flag, const uint8_t* inlier, int B, int N, int iters, double scale_px, double ftol, int min_rows,
                      double* work, float* pose_out, float* xyz, float* geom, float* cov_x, double* cov, double* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COPONERF_HIP_H */
