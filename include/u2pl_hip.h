/* libu2pl_hip.so -- C ABI of the MI355X-native U2PL training hot path.
 *
 * The reference (Haochen-Wang409/U2PL) is pure Python/PyTorch and has NO FFI of
 * its own; its replaceable seams are Python functions.  Each entry point below
 * names the reference code it replaces (file:line under the reference tree).
 * The Python seams that sit on top (u2pl_amd/, same names and argument meaning
 * as the reference) call these through ctypes -- see INTEGRATION.md.
 *
 * Conventions (every function):
 *   - returns 0 on success, a hipError_t value, or U2PL_EINVAL (1001);
 *   - never allocates, frees, synchronises or throws; the caller owns every
 *     buffer (device pointers unless stated) and passes the HIP stream;
 *   - tensors are float32 / int64 / uint32 as in the reference; "NCHW" means
 *     contiguous planar, "rows" means a (pixels, D) view with leading dim ld
 *     (NHWC activations), strides are in ELEMENTS.
 */
#ifndef U2PL_HIP_H
#define U2PL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#define U2PL_SEL_MAX_SLOTS 8 /* 2 order statistics per selection spec, <= 4 specs */
/* select workspace words (uint32): [0] n_valid  [1] n_total  [56+j] threshold j (float bits) */
#define U2PL_SEL_WORD_NVALID 0
#define U2PL_SEL_WORD_NTOTAL 1
#define U2PL_SEL_WORD_VAL 40
#define U2PL_SEL_WORD_THR 56

/* ---- reliability.hip ------------------------------------------------------ */
/* F.interpolate(mode="bilinear", align_corners=True): train_semi.py:320-322,345-350,355,372-374 */
int u2pl_bilinear_up_f32(const float* in, long sn, long sc, long sh, long sw, int N, int C, int h, int w,
                         float* out_nchw, int H, int W, hipStream_t stream);
/* autograd of the above for the student branches (train_semi.py:345-355 under loss.backward(), :527) */
int u2pl_bilinear_up_bwd_f32(const float* gout_nchw, int N, int C, int H, int W, float* gin, long sn, long sc,
                             long sh, long sw, int h, int w, hipStream_t stream);
/* F.softmax + torch.max -> (confidence, pseudo label): train_semi.py:323-324 */
int u2pl_pseudo_label_f32(const float* logits_nchw, int N, int C, int H, int W, float* conf, long long* label,
                          hipStream_t stream);
/* entropy = -sum(p*log(p+1e-10)); NaN where label==ignore; *nvalid += #valid:
 * train_semi.py:402-403, loss_helper.py:35-36 (label may be NULL) */
int u2pl_entropy_f32(const float* logits_nchw, const long long* label, int ignore, int N, int C, int H, int W,
                     float* entropy, unsigned* ws, hipStream_t stream);
/* same, fused with the bilinear up-sampling of the LOW-RES logits (train_semi.py:371-374 + 402-403):
 * the full-resolution logit tensor is never materialised; also accumulates ws[0] and the select's hist0 */
int u2pl_entropy_up_f32(const float* in, long sn, long sc, long sh, long sw, int N, int C, int h, int w, int H, int W,
                        const long long* label, int ignore, float* entropy, unsigned* ws, hipStream_t stream);
/* np.percentile(entropy[valid], q) x nspec (exact order statistics + numpy float32 lerp),
 * train_semi.py:405-407,412-415, loss_helper.py:38-40; spec kind 1 = OHEM k-th smallest
 * (loss_helper.py:521-526).  ws must be zeroed, then ws[0]=n_valid, ws[1]=n_total;
 * producers (u2pl_entropy*_f32, u2pl_ohem_prob_f32) also fill the pass-0 histogram (hist0_done=1). */
size_t u2pl_select_workspace_bytes(void);
int u2pl_select_f32(const float* values, long n, int nspec, const int* spec_kind_dev, const float* q32_dev,
                    const long long* kparam_dev, const float* fparam_dev, unsigned* ws, int hist0_done,
                    hipStream_t stream);
/* target[entropy >= thresh] = 255 and count of kept pixels: loss_helper.py:41-44 */
int u2pl_apply_drop_i64(const float* entropy, const unsigned* thr_bits, long long* target, int ignore, long n,
                        unsigned* nkept, hipStream_t stream);
/* low/high entropy masks, nearest down-sampling, label_onehot (batch-slot-0 quirk) as class
 * bitmasks for the concatenated batch: train_semi.py:408-465, utils.py:50-59 */
int u2pl_reliability_masks(const float* entropy, const unsigned* thr_lo_bits, const unsigned* thr_hi_bits,
                           const long long* label_l, const long long* label_u, int ignore, int B, int H, int W,
                           int h, int w, int negative_high_entropy, float* low_mask, float* high_mask,
                           unsigned* lbits, hipStream_t stream);
/* fused tail: unsup target overwrite + masks + class bits in one launch (thr_bits = {drop, low, high}) */
int u2pl_reliability_apply(const float* entropy, const unsigned* thr_bits, const long long* label_l,
                           const long long* label_u, int ignore, int B, int H, int W, int h, int w,
                           int negative_high_entropy, long long* target_u, unsigned* nkept, float* low_mask,
                           float* high_mask, unsigned* lbits, hipStream_t stream);
int u2pl_pack_class_bits(const long long* onehot, int N, int C, int h, int w, unsigned* bits, hipStream_t stream);
int u2pl_unpack_class_bits(const unsigned* bits, int N, int C, int h, int w, long long* onehot,
                           hipStream_t stream);

/* ---- contrast.hip --------------------------------------------------------- */
/* loss_helper.py:103-141 per-pixel masks (anchor / low-valid / negative) as class bitmasks */
int u2pl_contra_classify(const float* prob, long sn, long sc, long sp, const unsigned* lbits,
                         const float* low_mask, const float* high_mask, int N2, int num_labeled, int C, int h,
                         int w, float thr_p, float thr_n, int low_rank, int high_rank, unsigned* abits,
                         unsigned* lowbits, unsigned* nbits, void* compact_workspace, hipStream_t stream);
/* boolean-mask indexing order (loss_helper.py:115-116,119-123,142): idx int32 [3][32][cap] (plane 0 anchors,
   plane 2 negative keys; plane 1 (low-valid) is counted only), counts u32 [3][32].
   compact_workspace (u2pl_compact_workspace_bytes) handed to u2pl_contra_classify receives the per-block
   counts as a by-product; pass counted=1 to u2pl_compact_lists then (NULL / 0 otherwise). */
size_t u2pl_compact_workspace_bytes(long P);
int u2pl_compact_lists(const unsigned* abits, const unsigned* lowbits, const unsigned* nbits, long P, int C,
                       void* workspace, int* idx, long cap, unsigned* counts, int counted, hipStream_t stream);
/* torch.mean(rep_teacher[low_valid], dim=0): loss_helper.py:119-123 */
size_t u2pl_proto_workspace_bytes(long P, int C, int D);
int u2pl_class_prototypes(const float* rows, long ld, int D, const int* idx, long cap, const unsigned* counts,
                          int C, long P, void* workspace, float* proto, const unsigned* lowbits,
                          hipStream_t stream);
/* loss_helper.py:80-154 in THREE launches (classify + per-block counts; prototype streaming; ordered compaction write with
 * in-block offsets + list lengths merged with the ordered prototype finish): same outputs as u2pl_contra_classify +
 * u2pl_compact_lists + u2pl_class_prototypes.  rows: teacher features, row r at rows + r*ld. */
size_t u2pl_contra_phase1_workspace_bytes(long P, int C, int D);
int u2pl_contra_phase1(const float* prob, long sn, long sc, long sp, const unsigned* lbits, const float* low_mask,
                       const float* high_mask, int N2, int num_labeled, int C, int h, int w, float thr_p, float thr_n,
                       int low_rank, int high_rank, const float* rows, long ld, int D, unsigned* abits, unsigned* lowbits,
                       unsigned* nbits, int* idx, long cap, unsigned* counts, float* proto, void* workspace,
                       hipStream_t stream);
/* keys = rep_teacher[negative_mask]: loss_helper.py:142 */
int u2pl_gather_rows_f32(const float* rows, long ld, int D, const int* list, long n, float* out,
                         hipStream_t stream);
/* dequeue_and_enqueue FIFO (utils.py:27-47) on a device ring; tail=(head+len)%cap */
/* The bank as a device-resident object: state = int64 [C][5] {ring offset in `storage` (rows), cap, head, len,
 * ptr}; u2pl_bank_enqueue_f32 appends counts_dev[c] rows per class at the tails and advances the state with the
 * arithmetic of dequeue_and_enqueue (utils.py:27-47) -- no host-side lengths or heads needed.  idx == NULL: class c's
 * rows are rows[row_start_dev[c] + j]. */
size_t u2pl_bank_state_bytes(int C);
int u2pl_bank_init(long long* state, int C, const long long* caps_host, hipStream_t stream);
int u2pl_bank_enqueue_f32(long long* state, float* storage, int D, const float* rows, long ld, const int* idx,
                          long idx_stride, const long long* row_start_dev, const unsigned* counts_dev, int C,
                          hipStream_t stream);
int u2pl_bank_append_f32(float* bank, long cap, long tail, int D, const float* rows, long ld, const int* list,
                         long n_new, hipStream_t stream);
/* same for every class in ONE launch; desc_dev = int64 [nclass][6] {bank, cap, tail, rows, list|0, n_new} */
int u2pl_bank_append_multi_f32(const long long* desc_dev, int nclass, int D, long ld, long max_new,
                               hipStream_t stream);
/* cosine_similarity / temp + cross_entropy(target 0): loss_helper.py:173-230 */
size_t u2pl_infonce_job_bytes(void);
/* head (int [P], all -1 between calls), next (int [njobs*Q]), seg_len (int [njobs*Q], > 0 for the first entry of every
   group of entries of one job that sampled the same candidate; host-built) may all be NULL; when given, the group leaders
   that hit the same pixel are chained for u2pl_scatter_rows_ordered_f32 */
int u2pl_infonce_f32(const void* jobs_dev, int njobs, const float* rep, long ld, int D, int Q, int K,
                     float temp, float* loss_q, float* ganchor, int* anchor_pix, int* head, int* next,
                     const int* seg_len, hipStream_t stream);
/* u2pl_infonce_f32 + u2pl_infonce_reduce_f32 (+ u2pl_zero_rows_f32 of the rows the previous step's backward wrote: zero_*)
 * in ONE launch.  workspace: u2pl_infonce_fused_workspace_bytes bytes, zeroed once by the caller and reused.  Q % 4 == 0. */
size_t u2pl_infonce_fused_workspace_bytes(int njobs, int Q);
int u2pl_infonce_fused_f32(const void* jobs_dev, int njobs, const float* rep, long ld, int D, int Q, int K, float temp,
                           float* loss_q, float* ganchor, int* anchor_pix, int* head, int* next, const int* seg_len,
                           float* zero_dst, long zero_ld, const int* zero_pix, long zero_n, void* workspace,
                           float inv_valid_seg, float* loss, hipStream_t stream);
int u2pl_infonce_reduce_f32(const float* loss_q, int njobs, int Q, float inv_valid_seg, float* loss,
                            hipStream_t stream);
/* d loss / d rep (loss_helper.py:205-230 backward) without a dense zero fill and without float atomics: dst is a
   persistent all-zero (P, D) buffer; per sampled pixel dst[pix] = scale * gout * (sum of its entries' src rows in
   ascending entry order); head is re-armed to -1.  order / seg_pos / seg_len: host-built grouping of every job's entries
   by sampled candidate (see hipops.group_entries).  u2pl_zero_rows_f32 clears those rows again afterwards. */
int u2pl_scatter_rows_ordered_f32(float* dst, long ld, int D, const int* pix, const int* next, int* head,
                                  const int* order, const int* seg_pos, const int* seg_len, const float* src, long n,
                                  const float* gout_dev, float scale, hipStream_t stream);
int u2pl_zero_rows_f32(float* dst, long ld, int D, const int* pix, long n, hipStream_t stream);
/* Phase 2's sampling plan on the device (loss_helper.py:156-196; single rank, C <= 32, Q <= 1024): from the phase-1 list
 * lengths (counts_dev, uint32 [3][32]) and the device-resident bank state (after u2pl_bank_enqueue_f32) it writes what
 * the host builds after reading the lengths back: the valid classes (counts[1][c] > 0, loss_helper.py:156-158) and
 * their number, the jobs in class order (position i of the valid list has candidates and class valid[i] has keys,
 * loss_helper.py:176-178; the candidates are those of the POSITION, loss_helper.py:179), each job's descriptor
 * (u2pl_infonce_job_bytes), its index draws idx_out[j][Q + Q K] = words[j (Q + Q K) + k] % bound (torch.randint on the CPU
 * generator is raw mt19937 word % high, loss_helper.py:179-196; words: C (Q + Q K) raw words uploaded by the host), and
 * the anchors' grouping of hipops.group_entries (groups: int [3][C Q] order / seg_pos / seg_len).  anchor_pix [C Q]: -1
 * for the entries of absent jobs.  plan_hdr (u2pl_infonce_plan_hdr_bytes): {njobs, valid_seg, (float)(1 / valid_seg),
 * (float)(1 / (Q valid_seg)), njobs Q}; njobs = 0 when valid_seg <= 1 (loss_helper.py:160-162) and *loss = 0.0f.
 * mirror: uint32 [3 * 32 + 2] on the device = the counts, njobs, valid_seg, for the host to copy back when it likes. */
size_t u2pl_infonce_plan_hdr_bytes(void);
int u2pl_infonce_plan(const unsigned* counts_dev, const long long* bank_state, const unsigned* words, int C, int Q, int K,
                      const int* lists, long list_stride, const float* proto, int D, const float* storage, void* jobs_dev,
                      long long* idx_out, int* groups, int* anchor_pix, void* plan_hdr, unsigned* mirror, float* loss,
                      hipStream_t stream);
/* u2pl_infonce_fused_f32 (loss_helper.py:173-233) with the job count and 1 / valid_seg taken from plan_hdr: grid of
 * max_jobs jobs, blocks of absent jobs only clear their stale row; per-job buffers sized for max_jobs; same arithmetic
 * and summation order for the jobs that exist.  No job: *loss keeps the 0.0f u2pl_infonce_plan wrote. */
int u2pl_infonce_fused_dev_f32(const void* jobs_dev, const void* plan_hdr, int max_jobs, const float* rep, long ld, int D,
                               int Q, int K, float temp, float* loss_q, float* ganchor, int* anchor_pix, int* head,
                               int* next, const int* seg_len, float* zero_dst, long zero_ld, const int* zero_pix,
                               long zero_n, void* workspace, float* loss, hipStream_t stream);
/* u2pl_scatter_rows_ordered_f32 (loss_helper.py:205-230 backward) with n = njobs Q and scale = 1 / (Q valid_seg) taken
 * from plan_hdr; max_n = max_jobs Q sizes the grid */
int u2pl_scatter_rows_ordered_dev_f32(float* dst, long ld, int D, const int* pix, const int* next, int* head,
                                      const int* order, const int* seg_pos, const int* seg_len, const float* src,
                                      long max_n, const float* gout_dev, const void* plan_hdr, hipStream_t stream);

/* ---- losses.hip ----------------------------------------------------------- */
/* F.cross_entropy(ignore_index=255) fwd/bwd: loss_helper.py:46, 295-320, 531 */
size_t u2pl_ce_workspace_bytes(void);
int u2pl_ce_fwd_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H, int W,
                    int unsup_weight, void* workspace, float* out3, hipStream_t stream);
int u2pl_ce_bwd_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H, int W,
                    const float* out3_dev, const float* gout_dev, float gmul, float* grad, hipStream_t stream);
/* nn.CrossEntropyLoss(weight=class_weight, ignore_index, reduction="mean") of the `use_weight: True` criteria
   (loss_helper.py:265-292,461-488): loss = sum w[t]*l / sum w[t]; out3 = {loss, 1/sum w, sum w} */
int u2pl_ce_fwd_weighted_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H, int W,
                             const float* class_weight, void* workspace, float* out3, hipStream_t stream);
int u2pl_ce_bwd_weighted_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H, int W,
                             const float* class_weight, const float* out3_dev, const float* gout_dev, float gmul,
                             float* grad, hipStream_t stream);
/* OhemCrossEntropy2dTensor: loss_helper.py:502-531 */
int u2pl_ohem_prob_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H,
                       int W, float* mask_prob, unsigned* ws, hipStream_t stream);
int u2pl_ohem_apply_i64(const float* mask_prob, const unsigned* thr_bits, const long long* target, int ignore,
                        long n, long long* kept_target, hipStream_t stream);
/* validate(): argmax + intersection/output/target histograms (train_semi.py:620-641, utils.py:568-580) */
int u2pl_confusion_hist_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H, int W,
                            long long* hist3c, hipStream_t stream);

/* ---- infer.hip (prediction epilogue / prologue) ---------------------------- */
/* F.interpolate(output, (h, w), bilinear, align_corners=True) + torch.argmax(dim=1) + colorful(mask, colormap):
 * infer.py:127-130,137-142; eval.py:294-300 + utils.py:526-531 (colorize).  The interpolated values are the bits
 * u2pl_bilinear_up_f32 would store but are never written; lowest class index wins a tie (u2pl_confusion_hist_f32's rule).
 * label uint8 [N][H][W]; palette uint8 [256][3] and rgb uint8 [N][H][W][3] may both be NULL (labels only).
 * C > 256 returns 1001. */
int u2pl_predict_map_f32(const float* in, long sn, long sc, long sh, long sw, int N, int C, int h, int w, int H, int W,
                         unsigned char* label, const unsigned char* palette, unsigned char* rgb, hipStream_t stream);
/* (image - mean) / std + permute + F.interpolate(image, input_scale, bilinear, align_corners=True): infer.py:119-124.
 * img uint8 [h][w][3]; lut float [3][256] = the normalised value of every byte per channel (host: float64 expression
 * rounded once to fp32); out float [H][W][3], i.e. a (1,3,H,W) tensor in channels_last memory. */
int u2pl_infer_input_u8_f32(const unsigned char* img_hwc, int h, int w, const float* lut, float* out_hwc, int H, int W,
                            hipStream_t stream);
/* Test-time flip / probability fusion (the block eval.py:166-180 leaves commented out): one view's low-resolution logits
 * in [C][h][w] (through strides) are interpolated (bilinear, align_corners=True: the bits u2pl_bilinear_up_f32 would store)
 * to the hc x wc window at (h0, w0) of pred [C][H][W]; with flip the window pixel x takes column wc-1-x; with softmax the
 * C values of a pixel become exp(v - max) / sum (classes upward, ~1 ulp exponential); pred += weight * that; with bump
 * count [H][W] += 1 inside the window (count may be NULL when bump == 0).  One owner per element, no atomics.
 * NULL pred / in, NULL count with bump, C outside [1, 256], h or w < 1, a window not inside the accumulator: 1001. */
int u2pl_window_fuse_f32(float* pred, float* count, int C, int H, int W, const float* in, long sc, long sh, long sw, int h,
                         int w, int h0, int w0, int hc, int wc, int flip, int softmax, float weight, int bump,
                         hipStream_t stream);
/* Reliability maps on the prediction side: label and softmax entropy of every pixel from the low-resolution scores
 * [N][C][h][w] (through strides) in one launch; the full-resolution scores are never written (identity size h == H, w == W
 * is what the fused accumulators use).  label uint8 [N][H][W]: the bits u2pl_predict_map_f32 stores (infer.py:127-130, lowest
 * index wins a tie).  entropy float [N][H][W]: prob == 0, scores are logits: -sum(p * log(p)) of their softmax as
 * logf(s) - t / s (loss_helper.py:35-36, train_semi.py:402-403), the bits u2pl_entropy_up_f32 stores with label == NULL;
 * prob == 1, scores are non-negative class weights a_c (sums of softmaxes): p_c = a_c / S with S = sum a_c (classes upward),
 * -sum(p_c * logf(p_c)) over p_c > 0, and logf(C) where S <= 0; never NaN for finite input.
 * Does not touch a select workspace: run u2pl_select_f32 with hist0_done = 0 and ws[0] = ws[1] = N*H*W.
 * C outside [1, 256], a NULL pointer, h, w, H or W < 1: 1001. */
int u2pl_predict_entropy_f32(const float* in, long sn, long sc, long sh, long sw, int N, int C, int h, int w, int H, int W,
                             int prob, unsigned char* label, float* entropy, hipStream_t stream);
/* The drop rule of loss_helper.py:41-43 on uint8 maps, in place over n pixels: where thr_bits != NULL and
 * entropy[p] >= *thr_bits (float bits in device memory, e.g. a threshold word of the select workspace) label[p] = 255, and
 * *ndropped (may be NULL) gains the number of such pixels (integer atomics, one per block: deterministic).  Then, read after
 * the drop, rgb[p] = palette[label[p]] (palette uint8 [256][3], rgb uint8 [n][3]; both NULL: no colours) and, when
 * heat != NULL, heat[p] = clamp((int)(entropy[p] * heat_scale + 0.5f), 0, 255) with the product and the sum each rounded to
 * fp32.  NULL label / entropy, exactly one of palette / rgb NULL: 1001. */
int u2pl_reliable_map_u8(unsigned char* label, const float* entropy, const unsigned* thr_bits, long n,
                         const unsigned char* palette, unsigned char* rgb, unsigned char* heat, float heat_scale,
                         unsigned* ndropped, hipStream_t stream);
/* out[i] = lut256[in[i]] for n bytes of device memory (lut256: uint8 [256], device): the label maps of
 * u2pl_predict_map_f32 / u2pl_reliable_map_u8 in the dataset's raw ids (--raw_ids).  Any n, any alignment of in and out
 * (16-byte loads and stores between an unaligned head and tail); out == in is allowed, a partial overlap is not.
 * A NULL pointer: 1001. */
int u2pl_lut_u8(const unsigned char* in, unsigned char* out, long n, const unsigned char* lut256, hipStream_t stream);

/* ---- conv.hip (implicit GEMM on v_mfma_f32_32x32x2_f32) -------------------- */
/* nn.Conv2d forward (NHWC rows, weights [Cout][R][S][Cin]): resnet.py:25-41,178-186;
 * base.py:23-83; decoder.py:60-106,132-138.  Cin % 32 == 0 (3-channel stem: u2pl_im2col_f32) */
int u2pl_conv2d_fwd_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int N,
                        int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride,
                        int pad, int dil, hipStream_t stream);
/* forward + the train-mode BatchNorm statistics of its output in the conv epilogue (conv -> BN pairs:
 * resnet.py:120-140, base.py:23-83, decoder.py:60-106): per-tile pivot-shifted sums, finished by
 * u2pl_colreduce_finish_f32 */
int u2pl_conv2d_fwd_stat_blocks(int N, int Hout, int Wout, int Cout);
int u2pl_conv2d_fwd_bnstats_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy,
                                int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S,
                                int stride, int pad, int dil, const float* pivot, float* stats_partial,
                                hipStream_t stream);
int u2pl_colreduce_finish_f32(const float* partial, int nblk, int C, double* sums, hipStream_t stream);
/* forward + the EVAL-mode BatchNorm (+ residual, ReLU) that follows it, applied in the conv epilogue: the conv -> bn -> relu
 * (-> += identity) chains of resnet.py:118-138, base.py:23-83, decoder.py:60-106 when the model is in eval mode (teacher
 * pseudo-label pass train_semi.py:317-324, validate() :595-654, eval.py).  y = [relu]((conv + bias - mean) * invstd * gamma
 * + beta [+ res]) with the operation order of u2pl_bn_apply_f32, i.e. bit-identical to conv followed by that kernel.
 * res: [N*Hout*Wout][ldr] rows or NULL; Cout % 4 == 0 */
int u2pl_conv2d_fwd_bnact_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int N,
                              int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride,
                              int pad, int dil, const float* mean, const float* invstd, const float* gamma,
                              const float* beta, const float* res, long ldr, int relu, hipStream_t stream);
/* batch independent row-major GEMMs Y_z[M][Nn] = X_z[M][K] * W_z[Nn][K]^T on the fp32 matrix cores (element
   strides zx/zw/zy between the problems): the component products of the Winograd convolutions below */
int u2pl_gemm_batched_f32(const float* x, long ldx, long zx, const float* w, long zw, float* y, long ldy, long zy,
                          long M, int K, int Nn, int batch, hipStream_t stream);
/* Winograd F(mt x mt, 3x3), mt = 2 or 4, for nn.Conv2d(k=3, stride=1, padding=dil, dilation=dil) (resnet.py:25-41,
   base.py:54-83, decoder.py:60-106,132-138): V[a*a][tiles][C] <- x ; U[a*a][O][C] <- w ([O][3][3][C]);
   Mb[a*a][tiles][O] = V . U^T (u2pl_gemm_batched_f32) ; y <- Mb (+bias).  a = mt + 2, tiles = u2pl_wino_tiles.
   transposed = 1 builds U'[a*a][C][O] (taps rotated) for the data gradient.  stats_partial (rows =
   u2pl_wino_stat_blocks) receives the pivot-shifted BatchNorm column sums of y like u2pl_conv2d_fwd_bnstats_f32.
   Every transform moves 16 bytes per access: C % 4 == 0 (O % 4 == 0), and every row pitch (ldx, ldg, ldy, ldr) is a multiple
   of 4 floats, as for u2pl_absmax_f32 and the bnact forms -- U2PL_EINVAL before any launch otherwise.  Statistics need
   4 <= O <= 1024; u2pl_wino_stat_blocks returns 0 for O < 4. */
size_t u2pl_wino_tiles(int N, int H, int W, int dil, int mt);
int u2pl_wino_stat_blocks(long tiles, int O);
int u2pl_wino_input_f32(const float* x, long ldx, int N, int H, int W, int C, int dil, int mt, float* V,
                        hipStream_t stream);
int u2pl_wino_weight_f32(const float* w, int O, int C, int transposed, int mt, float* U, hipStream_t stream);
/* weight-gradient side: Mg[a*a][tiles][O] <- A dY A^T per tile ; batched P_z = Mg_z^T V_z over the tile rows
   (slabs [nsplit][O][a*a][C], nsplit = u2pl_wgrad_batched_splits) ; dw[O][3][3][C] (+)= G^T (sum of slabs) G */
int u2pl_wino_gy_f32(const float* gy, long ldg, int N, int H, int W, int O, int dil, int mt, float* Mg,
                     hipStream_t stream);
int u2pl_wgrad_batched_splits(long M, int Cin, int Cout, int batch);
size_t u2pl_wgrad_batched_workspace_bytes(long M, int Cin, int Cout, int batch);
int u2pl_wgrad_batched_f32(const float* dy, long lddy, long zdy, const float* x, long ldx, long zx, float* part,
                           long M, int Cin, int Cout, int batch, hipStream_t stream);
int u2pl_wino_wgrad_finish_f32(const float* part, int nsplit, int O, int C, int mt, int accumulate, float* dw,
                               hipStream_t stream);
int u2pl_wino_output_f32(const float* Mb, int N, int H, int W, int O, int dil, int mt, const float* bias, float* y,
                         long ldy, float* stats_partial, const float* pivot, hipStream_t stream);
/* Winograd form of u2pl_conv2d_fwd_bnact_f32: the output transform applies the eval-mode BatchNorm (+res, ReLU) */
int u2pl_wino_output_bnact_f32(const float* Mb, int N, int H, int W, int O, int dil, int mt, const float* bias, float* y,
                               long ldy, const float* mean, const float* invstd, const float* gamma, const float* beta,
                               const float* res, long ldr, int relu, hipStream_t stream);
/* BASELINE configs[4] ("config 5": reduced-precision student, fp32 EMA teacher / master weights): the same three
 * convolution products with the operands rounded to bf16 (RNE) while they are staged into LDS and multiplied on the
 * bf16 matrix cores (v_mfma_f32_32x32x16_bf16) with fp32 accumulation; every tensor in HBM stays fp32.  Arguments as the
 * f32 entry points above. */
int u2pl_conv2d_fwd_bf16op_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int N,
                               int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride,
                               int pad, int dil, hipStream_t stream);
int u2pl_conv2d_fwd_bnstats_bf16op_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy,
                                       int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S,
                                       int stride, int pad, int dil, const float* pivot, float* stats_partial,
                                       hipStream_t stream);
int u2pl_conv2d_dgrad_bf16op_f32(const float* dy, long lddy, const float* wT, float* dx, long lddx, int N, int Hin,
                                 int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad,
                                 int dil, hipStream_t stream);
int u2pl_conv2d_wgrad_bf16op_f32(const float* dy, long lddy, const float* x, long ldx, float* dw, void* workspace,
                                 int accumulate, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R,
                                 int S, int stride, int pad, int dil, hipStream_t stream);
/* autograd of nn.Conv2d under loss.backward() (train_semi.py:527): data and weight gradients */
int u2pl_conv2d_dgrad_f32(const float* dy, long lddy, const float* wT, float* dx, long lddx, int N, int Hin,
                          int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad,
                          int dil, hipStream_t stream);
int u2pl_weight_transpose_f32(const float* w, float* wt, int Cout, int RS, int Cin, hipStream_t stream);
size_t u2pl_conv2d_wgrad_workspace_bytes(int N, int Hout, int Wout, int Cin, int Cout, int R, int S);
int u2pl_conv2d_wgrad_f32(const float* dy, long lddy, const float* x, long ldx, float* dw, void* workspace,
                          int accumulate, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R,
                          int S, int stride, int pad, int dil, hipStream_t stream);
/* weight-gradient kernel choice under the split arithmetic (A/B switch; env U2PL_WGRAD_TR): 1 (default) = csrc/wgrad_tr.hip
 * (hardware-transposed LDS operand reads, layers with Cout, Cin >= 128), 0 = conv.hip's kernel.  Returns the previous value.
 * The workspace / slab-count queries above follow the switch: query and launch under the same setting. */
int u2pl_wgrad_set_tr(int on);
int u2pl_im2col_f32(const float* x, long ldx, float* col, int Kp, int N, int Hin, int Win, int Cin, int Hout,
                    int Wout, int R, int S, int stride, int pad, int dil, hipStream_t stream);

/* ---- gconv.hip (grouped convolution in exact fp32 on v_mfma_f32_16x16x4_f32) -------------------------------------
 * nn.Conv2d(groups > 1): the 3x3 of a ResNeXt bottleneck, resnet.py:25-36 (conv3x3 with groups) / :108-112 (Bottleneck width
 * and conv2).  Rows as in conv.hip (x / y / dy / dx are [N*H*W][ld], ld >= C: channel slices of wider buffers work); w is the
 * module's weight (Cout, Cin/groups, R, S) stored channels_last = [Cout][R][S][Cin/groups] -- the data gradient reads the SAME
 * tensor (no transposed or split operand).  Constraints (U2PL_EINVAL before any launch otherwise): Cin and Cout divisible by
 * groups; Cin/groups and Cout/groups multiples of 4 up to 64; stride 1 or 2; any dilation; R * S < 128, S <= 16; Hout / Wout the
 * convolution's output size; pointers 16-byte aligned and ld % 4 == 0.  fp32 products, fp32 accumulation, no atomics: the
 * weight gradient sums its pixel slabs in slab order, two runs give the same bits. */
/* forward (resnet.py:25-36, :108-112), bias optional (NULL) */
int u2pl_gconv2d_fwd_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int N, int Hin,
                         int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil,
                         int groups, hipStream_t stream);
/* autograd of that layer under loss.backward() (resnet.py:25-36, :108-112; train_semi.py:527): data gradient, stride 2 included */
int u2pl_gconv2d_dgrad_f32(const float* dy, long lddy, const float* w, float* dx, long lddx, int N, int Hin, int Win,
                           int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil, int groups,
                           hipStream_t stream);
/* weight gradient of that layer (resnet.py:25-36, :108-112): workspace = per-slab partial sums; accumulate: dw += instead of dw = */
size_t u2pl_gconv2d_wgrad_workspace_bytes(int N, int Hout, int Wout, int Cin, int Cout, int R, int S, int groups);
int u2pl_gconv2d_wgrad_f32(const float* dy, long lddy, const float* x, long ldx, float* dw, void* workspace,
                           int accumulate, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R,
                           int S, int stride, int pad, int dil, int groups, hipStream_t stream);

/* ---- dwconv.hip (depthwise 3x3 convolution in exact fp32: memory-bound stencils, no MFMA) ------------------------------
 * nn.Conv2d(C, C, 3, groups=C): the spatial half of an atrous separable convolution (the separable DeepLabv3+ decoder,
 * decoder.kwargs.separable; light plug-in encoders).  The reference project has no such layer: there is no reference line to
 * cite.  Argument lists are those of the gconv entry points above, and so is the layout: rows [N*H*W][ld], ld >= C (channel
 * slices of wider buffers work); w is the module's weight (C, 1, 3, 3) = [C][9], read by all three kernels (no derived operand).
 * Constraints (U2PL_EINVAL before any launch otherwise): groups == Cin == Cout (depth multiplier 1); C % 4 == 0; R == S == 3;
 * stride 1 or 2; pad >= 0 and dil >= 1, both up to 2^20 (a dilation larger than the image is fine: only the taps that land
 * inside contribute); Hout / Wout the convolution's output size; pointers (bias excepted) 16-byte aligned and ld % 4 == 0.
 * fp32 products, fp32 accumulation in tap order, no atomics: the weight gradient sums its pixel slabs in slab order, two runs
 * give the same bits. */
/* forward, bias optional (NULL) */
int u2pl_dwconv2d_fwd_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int N, int Hin,
                          int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil,
                          int groups, hipStream_t stream);
/* data gradient of that layer (gather form; stride 2 by a parity test on the tap coordinates) */
int u2pl_dwconv2d_dgrad_f32(const float* dy, long lddy, const float* w, float* dx, long lddx, int N, int Hin, int Win,
                            int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil, int groups,
                            hipStream_t stream);
/* weight gradient of that layer: workspace = per-slab partial sums (0: unsupported shape); accumulate: dw += instead of dw = */
size_t u2pl_dwconv2d_wgrad_workspace_bytes(int N, int Hout, int Wout, int Cin, int Cout, int R, int S, int groups);
int u2pl_dwconv2d_wgrad_f32(const float* dy, long lddy, const float* x, long ldx, float* dw, void* workspace,
                            int accumulate, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R,
                            int S, int stride, int pad, int dil, int groups, hipStream_t stream);

/* ---- operands.hip (the GEMM operands derived from the weights: piece planes, their maxima, activation maxima) ----------
 * The weights of the network change once per optimizer step (train_semi.py:526-528 optimizer.step(), :531-548 the EMA
 * teacher), the convolutions read them ~14 times per step (resnet.py:120-140 through the two student and two teacher
 * passes and the backward).  u2pl_weight_split3_f32 splits `batch` row-major fp32 matrices [rows][K] (K % 32 == 0, zw = rows * K
 * floats apart) ONCE into the three bf16 piece planes of the split-fp32 arithmetic, stored chunk-major in the image the GEMM's
 * LDS tile has: [K/32][3][Np][32] per matrix, the 16-byte segments of a row XOR-swizzled by (row >> 2) & 3 (csrc/ws_planes.h).
 * The matrices the GEMMs read:
 *   forward:        the [Cout][R*S*Cin] matrix (the weight itself, channels_last)
 *   data gradient:  the transposed [Cin][R*S*Cout] matrix (u2pl_weight_transpose_f32)
 *   Winograd:       the batch of a*a component matrices U[a*a][O][C] of u2pl_wino_weight_f32 (batch = a*a) */
size_t u2pl_weight_split3_bytes(int rows, int K, int batch);
int u2pl_weight_split3_f32(const float* w, long zw, int rows, int K, int batch, void* out, hipStream_t stream);
/* All bf16 weight splits / all Winograd filter transforms of a model in ONE launch each (after the optimizer / EMA update; the
 * per-weight entry points above remain the lazy path).  jobs: DEVICE arrays of
 *   struct { const float* src; unsigned short* out; long seg_begin; int rows, Np, K, kind, RS, batch; }   (48 bytes)
 *     kind 0: src = [batch][rows][K]; kind 1: src = conv weight [Cout][RS][Cin] read as [rows = Cin][K = RS * Cout] (the data
 *     gradient's operand); Np = u2pl_weight_split3_pad_rows(rows); seg_begin = prefix sum of batch * Np * K / 8; total = the sum
 *   struct { const float* w; float* U; long begin; int O, C, transposed, mt; }                             (40 bytes)
 *     begin = prefix sum of O * C; total = the sum.
 * Same bits as the per-weight calls. */
int u2pl_weight_split3_multi_f32(const void* jobs, int njobs, long total, hipStream_t stream);
int u2pl_weight_split3_pad_rows(int rows);
int u2pl_wino_weight_multi_f32(const void* jobs, int njobs, long total, hipStream_t stream);
/* The split-fp16 operands (the *_wsh_* entry points below; csrc/conv_geom.h).
 *   u2pl_weight_split2h_f32: the matrices of u2pl_weight_split3_f32 as planes [K/32][2][Np][32] fp16 + one uint32 per matrix (bit
 *     pattern of its max |w|) behind the planes of all of them, zero words up to a multiple of 16 bytes.  Three launches. */
size_t u2pl_weight_split2h_bytes(int rows, int K, int batch);
int u2pl_weight_split2h_f32(const float* w, long zw, int rows, int K, int batch, void* out, hipStream_t stream);
/* Every split-fp16 operand of a model rebuilt from the WEIGHTS in at most four launches (clear, maxima of every kind, pieces of
 * kinds 0 / 1, pieces of kinds 2 / 3; three where a table has no Winograd job): the bytes u2pl_weight_split2h_f32 writes for the same
 * operand -- for kinds 2 / 3 from the U of u2pl_wino_weight_f32 --, without an fp32 U in memory and with max |w| computed once per
 * weight.  jobs: DEVICE array of n_flat records of kinds 0 / 1 followed by n_wino records of kinds 2 / 3 (u2pl_weight_rebuild2h_job_bytes()
 * = 72 bytes each):
 *   struct { const float* src; unsigned short* out; long seg_begin; long amax_begin; unsigned* amax_dst;
 *            int rows, Np, K, kind, RS, mt; int mblk_begin, pblk_begin; }
 *     out: a u2pl_weight_split2h_bytes(rows, K, batch) buffer, batch = 1 (kinds 0 / 1) or (mt + 2)^2; Np = u2pl_weight_split3_pad_rows(rows)
 *     kind 0: src = [rows][K]; kind 1: src = conv weight [Cout][RS][Cin] read as [rows = Cin][K = RS * Cout].  seg_begin = prefix sum of
 *       Np * K / 8 (seg_total = the sum).  The jobs of one weight share its maximum: amax_dst = the word behind the planes of the
 *       weight's FIRST job in the table (out + the plane bytes), amax_begin = prefix sum of rows * K / 4 over first jobs (a further job
 *       of a weight carries the prefix reached so far: length 0; amax_total = the sum)
 *     kind 2: src = conv weight [O][3][3][C], planes of U[z][rows = O][K = C]; kind 3: planes of U'[z][rows = C][K = O] (rotated taps);
 *       mt = 2 or 4; C % 4 == 0.  mblk_begin / pblk_begin = prefix sums of ceil(O * C / 4 / span(1)) / ceil(Np * K / 8 / span(2)) with
 *       span = u2pl_weight_rebuild2h_span (wino_mblocks / wino_pblocks = the sums). */
int u2pl_weight_rebuild2h_job_bytes(void);
int u2pl_weight_rebuild2h_span(int which);
int u2pl_weight_rebuild2h_f32(const void* jobs, int n_flat, int n_wino, long seg_total, long amax_total, int wino_mblocks,
                              int wino_pblocks, hipStream_t stream);
/* "amax object" and u2pl_absmax_f32: see the split-fp16 section below */
int u2pl_amax_words(void);
int u2pl_absmax_f32(const float* x, long ld, long M, int C, float* out, int clear, hipStream_t stream);

/* ---- igemm_ws.hip (split-fp32 implicit GEMM with pre-split weights; round 4) -------------------------------------
 * The *_ws entry points are the conv.hip calls of the same name with a u2pl_weight_split3_f32 buffer in place of the fp32 weight
 * pointer.  Same arithmetic, same summation order as conv.hip's split kernels: results are bit-identical to u2pl_conv2d_fwd_f32 /
 * _bnstats / _bnact / u2pl_conv2d_dgrad_f32 / u2pl_gemm_batched_f32 under U2PL_CONV_SPLIT=1 (statistics partial sums
 * included; stats_partial has u2pl_igemm_ws_stat_blocks rows).  Cout > 64 only (narrower layers stay on conv.hip). */
int u2pl_igemm_ws_stat_blocks(int N, int Hout, int Wout);
/* launch shape of the ws kernel (A/B switch, same results; env U2PL_WS_PERSIST): 1 (default) = persistent, at most one
 * block per CU working through its tiles; 0 = one block per tile */
int u2pl_igemm_ws_set_persist(int on);
/* the tile plan a *_ws_* / *_wsh_* call of M output rows, reduction length K = R * S * Cin, Cout columns and `batch` matrices runs under
 * (host query, no launch; what u2pl_conv2d_fwd_stat_blocks is to conv.hip's planner).  np: pieces per operand, 3 = the *_ws_* calls,
 * 2 = *_wsh_*.  out[3] = {kind, wide tiles, narrow tiles}: kind 0 = 128 x 256 tiles only, 1 = 128 x 128 tiles only, 2 = mixed in one
 * launch (the full rounds as `wide` 128 x 256 tiles, the remainder as `narrow` 128 x 128 tiles), 3 = the same as two launches
 * (U2PL_WS_MIX2=1).  Follows U2PL_WS_NARROW, U2PL_WS_MIX2, U2PL_WS_FIX2 and u2pl_igemm_ws_set_persist like the launches do.
 * The query answers for the model alone and does not tell whether a call can be launched: K is used as K / 32 chunks (the launches
 * refuse Cin % 32 != 0), Cout <= 64 gets the narrow plan although the callers keep such layers on conv.hip, and pointers, pitches and
 * extents are not seen.  Refused (U2PL_EINVAL): a non-positive size, np other than 2 or 3, out == NULL, M >= 2^31 or 2^30 tiles. */
int u2pl_igemm_ws_plan(long M, int K, int Cout, int batch, int np, int* out);
int u2pl_conv2d_fwd_ws_f32(const float* x, long ldx, const void* wsplit, const float* bias, float* y, long ldy, int N,
                           int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad,
                           int dil, hipStream_t stream);
int u2pl_conv2d_fwd_bnstats_ws_f32(const float* x, long ldx, const void* wsplit, const float* bias, float* y, long ldy,
                                   int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S,
                                   int stride, int pad, int dil, const float* pivot, float* stats_partial,
                                   hipStream_t stream);
int u2pl_conv2d_fwd_bnact_ws_f32(const float* x, long ldx, const void* wsplit, const float* bias, float* y, long ldy, int N,
                                 int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride,
                                 int pad, int dil, const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, const float* res, long ldr, int relu, hipStream_t stream);
int u2pl_conv2d_dgrad_ws_f32(const float* dy, long lddy, const void* wTsplit, float* dx, long lddx, int N, int Hin,
                             int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil,
                             hipStream_t stream);
int u2pl_gemm_batched_ws_f32(const float* x, long ldx, long zx, const void* wsplit, float* y, long ldy, long zy, long M,
                             int K, int Nn, int batch, hipStream_t stream);

/* ---- split-fp16 (round 6; csrc/conv_geom.h): the same GEMMs with THREE fp16 piece products per fp32 product instead of six
 * bf16 ones.  Each operand is scaled per tensor by a power of two chosen from its largest magnitude (exact), split into two fp16
 * pieces (x s = h0 + h1 to 2^-25 |x s|) and multiplied as a1 b0 + a0 b1 + a0 b0 with fp32 accumulation; the accumulators are
 * scaled back with ldexp.  Replaces the same reference lines as the *_ws_* family above (u2pl/models/resnet.py:120-140,
 * base.py:54-100, decoder.py:60-142 forward; loss.backward() train_semi.py:527).
 *   "amax object": u2pl_amax_words() (= 2048) device floats, ZEROED by the caller before its producer runs -- 64 shards, one per
 *     128-byte line (same-line atomics serialise; tools/micro/atomic_shard.hip); the tensor's maximum is the maximum over the
 *     shards (bit patterns of |x|: NaN if any element is NaN).  Every x_amax / dy_amax / *_amax argument below is one.
 *   u2pl_absmax_f32: out <- max |x| over [M][C] (C % 4 == 0, ld % 4 == 0); clear != 0 zeroes the object first.  Any upper bound
 *     within ~2^8 of the true maximum keeps fp32-class accuracy; a value BELOW the maximum overflows fp16.
 *   u2pl_conv2d_fwd_bnact_wsh_f32's y_amax: NULL or an amax object for max |y| of the fused output (the next layer's x_amax). */
/* producers that leave the maximum of what they write (fused: no extra pass): the entry points of the same name without
 * `_amax` plus caller-ZEROED device floats that receive max |output| (bit-pattern atomicMax: deterministic; NULL = not wanted).
 * Reference lines as for the plain forms (BatchNorm base.py:6-8 forward / backward; Winograd transforms of resnet.py:25-41). */
int u2pl_bn_apply_amax_f32(const float* x, long ldx, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* res, long ldr, int relu, const float* drop, long rows_per_image, float* y, long ldy, long M,
                           int C, float* y_amax, hipStream_t stream);
int u2pl_bn_bwd_apply_amax_f32(const float* dy, long lddy, const float* x, long ldx, const float* y, long ldy, const float* mean,
                               const float* invstd, const float* gamma, const float* drop, long rows_per_image, const double* sums,
                               double count, float* dx, long lddx, float* dres, long lddr, long M, int C, const double* psums,
                               float* gsink, float* bsink, int accumulate, float* dx_amax, float* dres_amax, const float* relu_beta,
                               hipStream_t stream);
/* y = relu(BN(x)) without a residual: the backward's ReLU mask recomputed from x with the forward's own expression (same bits as
 * [y > 0]) instead of read from y -- u2pl_bn_bwd_sums_f32 / the apply above with y == NULL and relu_beta = the layer's beta */
int u2pl_bn_bwd_sums_mx_f32(const float* dy, long lddy, const float* x, long ldx, const float* mean, const float* invstd,
                            const float* gamma, const float* beta, const float* drop, long rows_per_image, long M, int C,
                            void* workspace, double* sums, hipStream_t stream);
/* y = relu(BN(x) + res): the mask cannot be recomputed from x, so the forward leaves it as a bit plane and the backward reads
 * the plane instead of y (1/32 of a stream).  unsigned bits[M][ldb], ldb >= C / 32: bit c % 32 of word [row][c / 32] = stored
 * y[row][c] > 0 (after residual, ReLU and Dropout2d scale; NaN: 0); words beyond C / 32 of a row are not touched.  C % 32 == 0,
 * else U2PL_EINVAL.  u2pl_bn_apply_bits_f32 = u2pl_bn_apply_amax_f32 (y_amax may be NULL) + the plane; the two backward entries
 * are u2pl_bn_bwd_sums_f32 / u2pl_bn_bwd_apply_amax_f32 with (bits, ldb) in the place of (y, ldy): the same bytes out.
 * u2pl_bn_apply_f32 / u2pl_bn_apply_amax_f32 with relu == 3 write the same plane packed behind y's last row, at
 * (unsigned*)(y + M * ldy) with ldb = C / 32: the caller's y buffer holds M * C / 32 more words. */
int u2pl_bn_apply_bits_f32(const float* x, long ldx, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* res, long ldr, int relu, const float* drop, long rows_per_image, float* y, long ldy, long M,
                           int C, float* y_amax, unsigned* bits, long ldb, hipStream_t stream);
int u2pl_bn_bwd_sums_bits_f32(const float* dy, long lddy, const float* x, long ldx, const unsigned* bits, long ldb,
                              const float* mean, const float* invstd, const float* drop, long rows_per_image, long M, int C,
                              void* workspace, double* sums, hipStream_t stream);
int u2pl_bn_bwd_apply_bits_f32(const float* dy, long lddy, const float* x, long ldx, const unsigned* bits, long ldb,
                               const float* mean, const float* invstd, const float* gamma, const float* drop, long rows_per_image,
                               const double* sums, double count, float* dx, long lddx, float* dres, long lddr, long M, int C,
                               const double* psums, float* gsink, float* bsink, int accumulate, float* dx_amax, float* dres_amax,
                               hipStream_t stream);
int u2pl_wino_input_amax_f32(const float* x, long ldx, int N, int H, int W, int C, int dil, int mt, float* V, float* v_amax,
                             hipStream_t stream);
int u2pl_wino_output_bnact_amax_f32(const float* Mb, int N, int H, int W, int O, int dil, int mt, const float* bias, float* y,
                                    long ldy, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                    const float* res, long ldr, int relu, float* y_amax, hipStream_t stream);
int u2pl_wino_gy_amax_f32(const float* gy, long ldg, int N, int H, int W, int O, int dil, int mt, float* Mg, float* mg_amax,
                          hipStream_t stream);
int u2pl_conv2d_fwd_wsh_f32(const float* x, long ldx, const float* x_amax, const void* wsplit, const float* bias, float* y, long ldy,
                            int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad,
                            int dil, hipStream_t stream);
int u2pl_conv2d_fwd_bnstats_wsh_f32(const float* x, long ldx, const float* x_amax, const void* wsplit, const float* bias, float* y,
                                    long ldy, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S,
                                    int stride, int pad, int dil, const float* pivot, float* stats_partial, hipStream_t stream);
int u2pl_conv2d_fwd_bnact_wsh_f32(const float* x, long ldx, const float* x_amax, const void* wsplit, const float* bias, float* y,
                                  long ldy, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S,
                                  int stride, int pad, int dil, const float* mean, const float* invstd, const float* gamma,
                                  const float* beta, const float* res, long ldr, int relu, float* y_amax, hipStream_t stream);
int u2pl_conv2d_dgrad_wsh_f32(const float* dy, long lddy, const float* dy_amax, const void* wTsplit, float* dx, long lddx, int N,
                              int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil,
                              hipStream_t stream);
int u2pl_gemm_batched_wsh_f32(const float* x, long ldx, long zx, const float* x_amax, const void* wsplit, float* y, long ldy, long zy,
                              long M, int K, int Nn, int batch, hipStream_t stream);
/* split-fp16 weight gradients (csrc/wgrad_tr.hip; autograd of nn.Conv2d under loss.backward(), train_semi.py:527): the calls
 * u2pl_conv2d_wgrad_f32 / u2pl_wgrad_batched_f32 with the device-scalar maxima of both operands; same workspace and slab plan;
 * only where u2pl_wgrad_h_eligible(Cin, Cout) (Cin, Cout >= 128) -- U2PL_EINVAL otherwise. */
int u2pl_wgrad_h_eligible(int Cin, int Cout);
int u2pl_conv2d_wgrad_h_f32(const float* dy, long lddy, const float* dy_amax, const float* x, long ldx, const float* x_amax, float* dw,
                            void* workspace, int accumulate, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R,
                            int S, int stride, int pad, int dil, hipStream_t stream);
int u2pl_wgrad_batched_h_f32(const float* dy, long lddy, long zdy, const float* dy_amax, const float* x, long ldx, long zx,
                             const float* x_amax, float* part, long M, int Cin, int Cout, int batch, hipStream_t stream);

/* ---- nn.hip ----------------------------------------------------------------- */
/* nn.SyncBatchNorm / BatchNorm2d (base.py:6-8 get_syncbn): statistics, apply (+residual, ReLU,
 * Dropout2d scale: resnet.py:120-140, decoder.py:79-104), backward; sums are double [2][C] so the
 * cross-rank exchange is one small all-reduce per layer */
size_t u2pl_colreduce_workspace_bytes(long Mseg, int nseg, int C);
int u2pl_bn_stats_f32(const float* x, long ld, long M, int C, const float* pivot, void* workspace, double* sums,
                      hipStream_t stream);
int u2pl_colsum_f32(const float* x, long ld, long Mseg, int nseg, int C, void* workspace, double* sums,
                    hipStream_t stream);
int u2pl_bn_bwd_sums_f32(const float* dy, long lddy, const float* x, long ldx, const float* y, long ldy,
                         const float* mean, const float* invstd, const float* drop, long rows_per_image, long M,
                         int C, void* workspace, double* sums, hipStream_t stream);
int u2pl_bn_finalize_f32(const double* sums, double count, const float* pivot, int C, float eps, float momentum,
                         float* mean, float* invstd, float* running_mean, float* running_var, hipStream_t stream);
int u2pl_bn_eval_invstd_f32(const float* running_var, int C, float eps, float* invstd, hipStream_t stream);
/* round 5 (fewer launches on the dependency chain conv -> statistics -> normalise; same arithmetic, same bits):
 *  u2pl_bn_finish_finalize_f32    u2pl_colreduce_finish_f32 + u2pl_bn_finalize_f32 in one launch (single-rank train mode:
 *                                 no all-reduce between them); partial = the conv epilogue's [nblk][2][C] float partial sums;
 *                                 sums_out (double [2C], may be NULL) receives what u2pl_colreduce_finish_f32 would write
 *  u2pl_bn_eval_invstd_multi_f32  u2pl_bn_eval_invstd_f32 for every BatchNorm of a model at once; jobs_dev: device array of
 *                                 u2pl_bn_eval_invstd_job_bytes() = 32-byte records {const float* running_var; float* invstd;
 *                                 int64 first_element; int32 C; float eps}, first_element = running sum of the previous C's,
 *                                 total = sum of C
 *  u2pl_bn_bwd_apply_pg_f32       u2pl_bn_bwd_apply_f32 + the two u2pl_sums_to_f32 calls of the layer's parameter gradients
 *                                 (dgamma = psums[C..2C), dbeta = psums[0..C), psums = the LOCAL backward sums) */
int u2pl_bn_finish_finalize_f32(const float* partial, int nblk, int C, double count, const float* pivot, float eps,
                                float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                                double* sums_out, hipStream_t stream);
size_t u2pl_bn_eval_invstd_job_bytes(void);
int u2pl_bn_eval_invstd_multi_f32(const void* jobs_dev, int njobs, long total, hipStream_t stream);
int u2pl_bn_apply_f32(const float* x, long ldx, const float* mean, const float* invstd, const float* gamma,
                      const float* beta, const float* res, long ldr, int relu, const float* drop,
                      long rows_per_image, float* y, long ldy, long M, int C, hipStream_t stream);
int u2pl_bn_bwd_apply_f32(const float* dy, long lddy, const float* x, long ldx, const float* y, long ldy,
                          const float* mean, const float* invstd, const float* gamma, const float* drop,
                          long rows_per_image, const double* sums, double count, float* dx, long lddx, float* dres,
                          long lddr, long M, int C, hipStream_t stream);
int u2pl_bn_bwd_apply_pg_f32(const float* dy, long lddy, const float* x, long ldx, const float* y, long ldy,
                             const float* mean, const float* invstd, const float* gamma, const float* drop,
                             long rows_per_image, const double* sums, double count, float* dx, long lddx, float* dres,
                             long lddr, long M, int C, const double* psums, float* gsink, float* bsink, int accumulate,
                             hipStream_t stream);
int u2pl_sums_to_f32(const double* sums, int n, float scale, int accumulate, float* out, hipStream_t stream);
/* nn.MaxPool2d(3,2,1,ceil_mode=True): resnet.py:189-191 */
int u2pl_maxpool3s2_fwd_f32(const float* x, long ldx, int N, int H, int W, int C, int Ho, int Wo, float* y, long ldy,
                            unsigned char* tap, hipStream_t stream);
int u2pl_maxpool3s2_bwd_f32(const float* dy, long lddy, const unsigned char* tap, int N, int H, int W, int C, int Ho,
                            int Wo, float* dx, long lddx, hipStream_t stream);
/* Pyramid pooling (csrc/pool.hip): nn.AdaptiveAvgPool2d((b, b)) of x [N*H*W][C] (pitch ldx) for up to four levels b0..b3
   (each >= 1; 0 = level unused, its pointer ignored), all levels in one launch; level l writes y_l [N*b*b][C] (pitch ldy_l).
   Window rule (torch's), per axis: window i of b over H is [floor(i*H/b), ceil((i+1)*H/b)); neighbouring windows share a row
   when H % b != 0; b may exceed H.  The mean divides the fp32 sum by the true window area.  C % 4 == 0, pitches multiples of
   4 and >= C, bases 16-byte aligned, levels <= 16384, H and W <= 65535, N*H*W < 2^31; 1001 before any launch for C % 4, a
   level < 0, all levels 0, a null x or a null y of a used level.  Fixed summation order (first comment block of csrc/pool.hip): the same bits on every run. */
int u2pl_pyramid_pool_fwd_f32(const float* x, long ldx, int N, int H, int W, int C, int b0, int b1, int b2, int b3,
                              float* y0, long ldy0, float* y1, long ldy1, float* y2, long ldy2, float* y3, long ldy3,
                              hipStream_t stream);
/* its backward, a gather: dx[p] = sum over levels (in argument order; a null g_l is skipped) of sum over the windows (i, j)
   that contain pixel p, ascending, of g_l[window] * (1.0f / area(window)), then + add[p] when add is not null (the gradient x
   receives from its other consumer, pitch ldadd).  The windows of a level that contain row h are the range
   floor(h*b/H) .. ceil((h+1)*b/H) - 1.  dx [N*H*W][C] (pitch lddx) is written exactly once; no atomics, no memset.
   1001 before any launch for C % 4, a level < 0, all levels 0 or a null dx. */
int u2pl_pyramid_pool_bwd_f32(const float* g0, long ldg0, const float* g1, long ldg1, const float* g2, long ldg2,
                              const float* g3, long ldg3, const float* add, long ldadd, int N, int H, int W, int C,
                              int b0, int b1, int b2, int b3, float* dx, long lddx, hipStream_t stream);
/* Object-contextual representations (csrc/ocr.hip; OCRNet, Yuan et al. 2020).  Channel-wide tensors are NHWC rows: x, add, dx
   [N*HW][C]; q, g_y, y, dq [N*HW][D]; region-side f, g_f [N*K][C] and kk, v, dk, dv [N*K][D] (a [N, C, K, 1] activation).  K-wide
   tensors s, m, ds, w are [N*HW][K].  1 <= K <= 255, C % 4 == 0 (D likewise), N*HW < 2^31.  Channel-wide tensors: pitch a
   multiple of 4 and >= the row width, base 16-byte aligned (float4 accesses).  K-wide tensors are accessed by single floats:
   any pitch >= K (class logits of 19 classes come with pitch 19).  ws: caller-allocated floats, 16-byte aligned, at least what
   the _ws_floats query of the entry point returns (0 for a shape out of contract); its contents on entry do not matter.  A
   violation returns 1001 before any launch and leaves the outputs untouched.  Exact fp32, fixed summation order (first comment
   block of csrc/ocr.hip), no atomics, no memset: the same bits on every run.
   region pool forward ("spatial gather"): m[n,p,k] = softmax over the pixels p of image n of scale * s[n,p,k] (max-subtracted),
   f[n,k,:] = sum_p m[n,p,k] x[n,p,:].  Both are written. */
size_t u2pl_region_pool_fwd_ws_floats(int N, int HW, int K, int C);
int u2pl_region_pool_fwd_f32(const float* s, long lds, const float* x, long ldx, float scale, int N, int HW, int K, int C,
                             float* m, long ldm, float* f, long ldf, float* ws, hipStream_t stream);
/* its backward: dx[n,p,:] = sum_k m[n,p,k] g_f[n,k,:] (+ add[n,p,:], the gradient x receives from its other consumer; null: none),
   written exactly once; ds[n,p,k] = scale * m[n,p,k] * (g_f[n,k,:] . x[n,p,:] - c[n,k]), c[n,k] = g_f[n,k,:] . f[n,k,:] (equal to
   sum_p m (g_f . x): one pass over the pixels).  m and f are the forward's outputs.  A null g_f (no gradient reached f) gives
   dx = add (or 0) and ds = 0; x and f are then not read.  dx or ds may be null (that output is skipped), not both. */
size_t u2pl_region_pool_bwd_ws_floats(int N, int HW, int K, int C);
int u2pl_region_pool_bwd_f32(const float* g_f, long ldg, const float* m, long ldm, const float* x, long ldx, const float* f,
                             long ldf, const float* add, long ldadd, float scale, int N, int HW, int K, int C, float* dx,
                             long lddx, float* ds, long ldds, float* ws, hipStream_t stream);
/* region attention forward: w[n,p,:] = softmax over k of scale * q[n,p,:] . kk[n,k,:], y[n,p,:] = sum_k w[n,p,k] v[n,k,:].  Both
   are written.  No workspace. */
int u2pl_region_attn_fwd_f32(const float* q, long ldq, const float* kk, long ldk, const float* v, long ldv, float scale, int N,
                             int HW, int K, int D, float* w, long ldw, float* y, long ldy, hipStream_t stream);
/* its backward, from g_y and the saved w: dv[n,k,:] = sum_p w g_y; dw = g_y . v; e = scale * w * (dw - sum_k w dw);
   dq[n,p,:] = sum_k e kk[n,k,:]; dk[n,k,:] = sum_p e q[n,p,:].  Each of dq, dk, dv may be null (skipped), not all three; q is
   read only for dk. */
size_t u2pl_region_attn_bwd_ws_floats(int N, int HW, int K, int D);
int u2pl_region_attn_bwd_f32(const float* g_y, long ldg, const float* w, long ldw, const float* q, long ldq, const float* kk,
                             long ldk, const float* v, long ldv, float scale, int N, int HW, int K, int D, float* dq, long lddq,
                             float* dk, long lddk, float* dv, long lddv, float* ws, hipStream_t stream);
/* Criss-cross attention (csrc/ccattn.hip; CCNet, Huang et al. 2019).  Every pixel p = (y, x) of an image
   attends to its cross X(p): the W pixels of its row and the H - 1 other pixels of its column, L = H + W - 1 members.  All
   maps are NHWC rows: q, k, dq, dk [N*H*W][D]; v, res, out, g, dv [N*H*W][C]; pitch a multiple of 4 and >= the row width, base
   16-byte aligned (float4 accesses).  w is [N*H*W][L], single floats, any pitch >= L.  SLOT LAYOUT of w: for the pixel (y, x),
   slot j < W is the row member (y, j) (the pixel itself is slot x) and slot W + i - (i > y) is the column member (i, x), i != y.
   gamma is ONE float in device memory and is read on the device only (a graph replay sees the value SGD left there); scale is
   a host float.
   CONTRACT.  1001 before any launch, the outputs untouched, for: N, H or W < 1; D or C < 4 or not a multiple of 4;
   H + W - 1 > 512 (CC_MAX_L: the map is too large for one cross; tiling a cross is out of scope); N*H*W >= 2^31; a null q, k,
   v, gamma, w, out (forward) or g, w, gamma, ws (backward); a pitch below the row width, a channel-wide pitch that is not a
   multiple of 4 or a base that is not 16-byte aligned; all of dq, dk, dv, dgamma null.  The backward reads k only for dq, q only
   for dk and v only for dq, dk or dgamma: an operand that is not read may be null.
   ARITHMETIC.  Exact fp32 on the vector ALU in a fixed order (first comment block of csrc/ccattn.hip), no atomics, no memset,
   no U2PL_CONV_* switch applies: the same bits on every run, eager or replayed.  __fmaf_rn (one rounding): every step of a dot
   product's chain over the channels, every step of a weighted sum's chain over the cross members, the lanes' chains of s[p],
   and the forward's finish out = fma(gamma, sum, res).  Rounded apart: scale * dot, u - max, e / Z, the sums of Z, s and
   dgamma, scale * gamma, (scale gamma) * w, t - s, their product, gamma * sum (no res; dv).
   forward: w[p, m] = softmax over m in X(p) of scale * q[p] . k[m] (max-subtracted); out[p] = res[p] + gamma * sum_m w[p, m] v[m]
   (res null: gamma * sum).  w and out are both written.  No workspace. */
int u2pl_cc_attn_fwd_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* res,
                         long ldr, const float* gamma, float scale, int N, int H, int W, int D, int C, float* w, long ldw,
                         float* out, long ldo, hipStream_t stream);
/* its backward, from g = d out and the saved w: t[p, m] = g[p] . v[m], s[p] = sum_m w t, e = scale gamma w (t - s);
   dq[p] = sum_{m in X(p)} e[p, m] k[m]; dk[m] = sum_{p in X(m)} e[p, m] q[p] and dv[m] = gamma sum_{p in X(m)} w[p, m] g[p] (gathers
   over the target's own cross with the weight the SOURCE p gives to m, each row written once); dgamma[0] = sum_{n, p} s[p] (one
   float, written, not accumulated).  The gradient of res is g itself and is not this call's business.  Each of dq, dk, dv,
   dgamma may be null (skipped), not all four.  ws: u2pl_cc_attn_bwd_ws_floats floats (0 for a shape out of contract), 16-byte
   aligned; it holds t / e and the per-pixel s; its contents on entry do not matter. */
size_t u2pl_cc_attn_bwd_ws_floats(int N, int H, int W, int D, int C);
int u2pl_cc_attn_bwd_f32(const float* g, long ldg, const float* w, long ldw, const float* q, long ldq, const float* k, long ldk,
                         const float* v, long ldv, const float* gamma, float scale, int N, int H, int W, int D, int C,
                         float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, float* dgamma, float* ws,
                         hipStream_t stream);
/* Dense (non-local) attention, several heads (csrc/attn.hip; Non-local networks, Wang et al. 2018).  Per
   image n and head h: S = scale q_h k_h^T ([Pq][Pk], never in memory), P = softmax over the keys, o_h = P v_h,
   lse = max_j S + log sum_j exp(S - max) (natural log).  Rows: q, dq [N*Pq][heads*D]; k, dk [N*Pk][heads*D]; v, dv
   [N*Pk][heads*Dv]; o, g [N*Pq][heads*Dv]; head h owns the columns h*D .. / h*Dv ..; pitch a multiple of 4 and >= the row
   width, base 16-byte aligned (float4 accesses).  lse is dense: lse[(n*heads + h)*Pq + p].  scale is a host float.
   CONTRACT.  1001 before any launch, the outputs untouched, for: N, heads, Pq or Pk < 1; D outside 4 .. 128 or not a multiple
   of 4; Dv outside 4 .. 512 or not a multiple of 4; N*heads*Pq, N*Pq or N*Pk >= 2^31; a null q, k, v, o, lse (forward) or g, q,
   k, lse, ws (backward); a pitch below the row width or not a multiple of 4, a base that is not 16-byte aligned; all of dq, dk,
   dv null.  There is no cap on Pq or Pk.  The backward reads v and o only for dq or dk: with both null they may be null.
   ARITHMETIC.  Exact fp32, the products on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain), softmax, rescale and delta on the
   vector ALU, in a fixed order that depends on the shapes alone (ARITHMETIC CONTRACT block of csrc/attn.hip): keys in tiles of
   64 ascending with an online softmax (running maximum, one rescale of the sums per tile), one IEEE division at the end; no
   atomics, no memset, no host read, fixed launch sizes: the same bits on every run, eager or replayed.  Nothing of size
   Pq x Pk is written: the backward recomputes P = exp(S - lse).
   forward: writes o and lse.  The workspace query is 0 for every shape; ws is not read and may be null. */
size_t u2pl_attn_fwd_ws_floats(int N, int heads, int Pq, int Pk, int D, int Dv);
int u2pl_attn_fwd_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float scale, int N, int heads,
                      int Pq, int Pk, int D, int Dv, float* o, long ldo, float* lse, float* ws, hipStream_t stream);
/* its backward, from g = d o and the forward's o and lse: delta[p, h] = g[p, h, :] . o[p, h, :], dP = g v^T,
   dS = P o (dP - delta); dq = scale dS k; dk = scale dS^T q; dv = P^T g.  Each of dq, dk, dv may be null (skipped), not all
   three.  dq comes from blocks that own 64 queries and walk the key tiles ascending; dk and dv from blocks that own 64 keys and
   walk the query tiles ascending; with few key tiles the queries are cut into slabs whose partial sums are added in slab order.
   ws: u2pl_attn_bwd_ws_floats floats (0 for a shape out of contract), 16-byte aligned; it holds delta and the slab partials
   (O(rows x channels x slabs)); its contents on entry do not matter. */
size_t u2pl_attn_bwd_ws_floats(int N, int heads, int Pq, int Pk, int D, int Dv);
int u2pl_attn_bwd_f32(const float* g, long ldg, const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                      const float* o, long ldo, const float* lse, float scale, int N, int heads, int Pq, int Pk, int D, int Dv,
                      float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, float* ws, hipStream_t stream);
/* torch.cat / slices (base.py:99, decoder.py:117), 1x1 -> HxW bilinear broadcast (base.py:92-94) */
int u2pl_copy_rows_f32(const float* src, long lds, float* dst, long ldd, long M, int C, int accumulate,
                       hipStream_t stream);
int u2pl_copy_cols_f32(const float* src, long lds, float* dst, long ldd, long M, int C, hipStream_t stream);
int u2pl_broadcast_rows_f32(const float* v, long ldv, float scale, float* dst, long ldd, long rows_per_image, long M,
                            int C, hipStream_t stream);
/* F.interpolate(bilinear, align_corners=True) on feature maps: decoder.py:114-116 */
int u2pl_bilinear_rows_fwd_f32(const float* x, long ldx, int N, int h, int w, int C, int H, int W, float* y, long ldy,
                               hipStream_t stream);
int u2pl_bilinear_rows_bwd_f32(const float* dy, long lddy, int N, int h, int w, int C, int H, int W, float* dx,
                               long lddx, hipStream_t stream);
/* F.softmax(pred_all_teacher, dim=1): train_semi.py:365 */
int u2pl_softmax_rows_f32(const float* x, long ldx, float* y, long ldy, long M, int C, hipStream_t stream);
/* torch.optim.SGD step on a flat arena with 3 lr segments (lr_helper.py:18-19, train_semi.py:100-112,528)
 * and the teacher EMA (train_semi.py:531-548) */
int u2pl_sgd_step_f32(float* p, const float* g, float* buf, long n, long b1, long b2, float lr0, float lr1, float lr2,
                      float momentum, float weight_decay, int first, float grad_scale, hipStream_t stream);
int u2pl_ema_update_f32(float* t, const float* s, long n, float decay, float one_minus_decay, hipStream_t stream);
/* torch.optim.Adam step (lr_helper.py:20-21; amsgrad off) on the same arena layout: bias_correction1 = 1 - beta1^t,
 * bias_correction2_sqrt = sqrt(1 - beta2^t) for the step count t kept by the host.  one_minus_beta1 / one_minus_beta2 are
 * the host's (float)(1.0 - (double)beta), rounded once as torch's scalar weights are (like one_minus_decay above): the
 * device never forms 1.0f - beta, which at beta2 = 0.999 is 0.0009999871 instead of float(0.001).  beta1 is part of the call
 * for the record of the hyper-parameters only: exp_avg is updated as m += one_minus_beta1 * (g - m) */
int u2pl_adam_step_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, long b1, long b2, float lr0,
                       float lr1, float lr2, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                       float eps, float weight_decay, float bias_correction1, float bias_correction2_sqrt,
                       float grad_scale, hipStream_t stream);
/* The whole reliability split in ONE persistent launch (csrc/relfused.hip): bilinear up-sampling + entropy of the
 * train-mode teacher logits (train_semi.py:371-374,402), exact np.percentile thresholds (loss_helper.py:38-40,
 * train_semi.py:405-415), unsup target overwrite (loss_helper.py:41-43), low / high masks + nearest down-sampling +
 * label_onehot class bits (train_semi.py:408-465, utils.py:50-59).  nspec = 1 (target only) or 3; q32_host = HOST
 * array of percentiles/100 in float32.  workspace (u2pl_reliability_fused_workspace_bytes(G) bytes) is zeroed ONCE and
 * reused; epoch = number of earlier launches on it (barrier counters grow monotonically, totals alternate by parity);
 * thresholds are left in workspace words 16..18 (float bits), #kept in word 2.  G = power of two <= #CUs, <= 256.
 * cand: u2pl_reliability_fused_cand_floats(B*H*W, G) floats of scratch.  Every block publishes its entropies sorted by
 * histogram bin, so the members of the bins that hold the ranks are gathered after ONE device-wide barrier; only when
 * those bins hold more values than fit in LDS (all-equal entropies, heavy ties) a second barrier is used (workspace word
 * 4 counts launches, word 5 those that needed it).  flags bit 0: put an agent-scope release / acquire fence pair around
 * the barrier (the published data are written through and read past the L1 already: off by default).
 * Returns 1001 when the shape is not covered (fall back to entropy_up + select + reliability_apply). */
/* kernel launches issued by this library so far (host counter; bench.py: kernel launches per step vs C-ABI calls) */
size_t u2pl_kernel_launches(void);
/* Arithmetic of the fp32 convolution / GEMM entry points: 1 (default; env U2PL_CONV_SPLIT) = every fp32 operand split
 * exactly into three bf16 pieces and the six significant piece products accumulated in fp32 on the bf16 matrix cores
 * (fp32-class accuracy, csrc/conv.hip BF == 3); 0 = v_mfma_f32_32x32x2_f32.  set returns the previous value. */
int u2pl_conv_set_split(int on);
int u2pl_conv_get_split(void);
/* (debug) arm per-block start / end stamps of the three phase-1 kernels: buf = device uint32 [3][4096][2] in 100 MHz
 * ticks (kernel 0 classify, 1 prototype stream, 2 tail); NULL disarms.  Only in a -DU2PL_P1_DBG build of the library
 * (U2PL_EINVAL otherwise); tools/bench_phase1_blocks.py reads it. */
int u2pl_debug_phase1_times(unsigned* buf);
size_t u2pl_reliability_fused_workspace_bytes(int G);
size_t u2pl_reliability_fused_cand_floats(long n_px, int G);
int u2pl_reliability_fused(const float* logits_low, long sn, long sc, long sh, long sw, int B, int C, int h, int w,
                           int H, int W, const long long* label_u, const long long* label_l, int ignore, int nspec,
                           const float* q32_host, int negative_high_entropy, int hm, int wm, float* entropy,
                           long long* target_u, float* low_mask, float* high_mask, unsigned* lbits,
                           unsigned* workspace, float* cand, int G, unsigned epoch, int flags, hipStream_t stream);
/* generate_unsup_data(mode="cutmix"): augmentation.py:498-541 */
int u2pl_cutmix_f32(const float* img, const long long* label, const float* conf, const int* boxes_dev, int B, int C,
                    int H, int W, float* out_img, long long* out_label, float* out_conf, hipStream_t stream);

/* nn.Conv2d(kernel_size=1) on a 1x1 map (ASPP image-pooling branch, base.py:24-28): y[m][o] = x[m][:] . w[o][:] + bias[o]
   for M <= 16 rows, accumulated in float64 (the 2-sample BatchNorm behind it amplifies y's relative error ~50x) */
int u2pl_dense_small_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int M, int K,
                         int Cout, hipStream_t stream);
/* generate_unsup_data(mode="cutout" -> mode 1, boxes) / (mode="classmix" -> mode 2, sel): augmentation.py:486-541.
   sel_dev: uint64 [B], bit c set = class c of image i is in generate_class_mask's selected half */
int u2pl_strong_aug_f32(const float* img, const long long* label, const float* conf, const int* boxes_dev,
                        const unsigned long long* sel_dev, int mode, int B, int C, int H, int W, float* out_img,
                        long long* out_label, float* out_conf, hipStream_t stream);
/* torch.unique(pseudo_labels) (augmentation.py:488) as a per-image presence bitmask; bits [B] zeroed by the caller */
int u2pl_label_presence_i64(const long long* label, int B, long HW, unsigned long long* bits, hipStream_t stream);

/* sliding-window evaluation accumulators (eval.py:184-224): pred [C][H][W] += src [C][hc][wc] at (h0, w0), count += 1;
   then pred /= count */
int u2pl_window_accumulate_f32(float* pred, float* count, int C, int H, int W, const float* src, int h0, int w0,
                               int hc, int wc, hipStream_t stream);
int u2pl_window_normalize_f32(float* pred, const float* count, int C, int H, int W, hipStream_t stream);

/* device-side training data pipeline (augmentation.py:51-266 as composed by cityscapes.py:47-77): ToTensor, Normalize,
   RandResize (bilinear align_corners=False / legacy nearest), flip, zero-padded crop fused into one gather from the
   decoded uint8 sample.  img uint8 [B][H][W][3], lab uint8 [B][H][W], params int32 [B][8] = {rh, rw, flip, pad_top,
   pad_left, crop_y, crop_x, 0} (device); mean3 / std3 are HOST pointers to three floats. */
int u2pl_augment_u8_f32(const unsigned char* img, const unsigned char* lab, const int* params, int B, int H, int W,
                        int Sh, int Sw, const float* mean3, const float* std3, float* out_img, long long* out_lab,
                        hipStream_t stream);

/* the same pipeline with the reference's two remaining transform options and batches of mixed image sizes
   (augmentation.py:269-346 as composed by pascal_voc.py:48-71): ... RandResize -> RandRotate -> RandomGaussianBlur ->
   flip -> crop.  One record of U2PL_AUG_REC int32 per sample (device):
     [0] rh  [1] rw          size after RandResize (= H, W without it)
     [2] flip                0 / 1
     [3] pad_top [4] pad_left  zero padding of the crop (label 0 there)
     [5] crop_y  [6] crop_x    crop origin in the padded frame
     [7] flags               U2PL_AUG_ROTATE | U2PL_AUG_BLUR: what THIS sample gets (blur is a per-sample coin)
     [8] H  [9] W            size of the decoded sample (read when offsets != NULL)
     [10..13] m00 m01 m10 m11  bit patterns of the float32 rotation matrix handed to F.affine_grid
                             ([[cos a, sin a], [-sin a, cos a]], translation 0); ignored without U2PL_AUG_ROTATE
     [14] [15] 0
   img / lab: uint8, sample b starts at pixel offsets[b] (img: 3 bytes per pixel, [H_b][W_b][3]; lab: [H_b][W_b]);
   offsets == NULL: dense [B][H][W] layout, every sample H x W (the arguments; record words 8 and 9 are not read).
   mode: U2PL_AUG_ROTATE / U2PL_AUG_BLUR set when the CONFIG enables the option (any sample of the batch may carry the
   flag).  With U2PL_AUG_BLUR the call runs two passes through `scratch` (u2pl_augment_ex_scratch_bytes, fp32) and reads
   blur_w, 25 float32 weights [ky][kx] on the device; otherwise both may be NULL.  Rotated-out pixels: image 0, label
   ignore_label.  mean3 / std3 are HOST pointers.  Mode 0 on a dense batch gives the bits of u2pl_augment_u8_f32. */
#define U2PL_AUG_REC 16
#define U2PL_AUG_ROTATE 1
#define U2PL_AUG_BLUR 2
size_t u2pl_augment_ex_scratch_bytes(int B, int Sh, int Sw, int mode);
int u2pl_augment_ex_u8_f32(const unsigned char* img, const unsigned char* lab, const long long* offsets,
                           const int* records, int B, int H, int W, int Sh, int Sw, int ignore_label, int mode,
                           const float* mean3, const float* std3, const float* blur_w, float* scratch, float* out_img,
                           long long* out_lab, hipStream_t stream);
/* u2pl_augment_ex_u8_f32 with dataset.label_map fused into the label read: every SOURCE label byte v becomes lut256[v]
   (uint8 [256] on the device; the host validates that each entry is < num_classes or == ignore_label, so no other value
   can reach a loss kernel whatever the files hold).  The map applies at load, before any transform: the crop's padding
   still writes 0 and rotated-out pixels ignore_label, both in mapped space, neither looked up.  Image output: the bits of
   u2pl_augment_ex_u8_f32; with the identity table the labels too.  lut256 == NULL: 1001. */
int u2pl_augment_lut_u8_f32(const unsigned char* img, const unsigned char* lab, const long long* offsets,
                            const int* records, int B, int H, int W, int Sh, int Sw, int ignore_label, int mode,
                            const unsigned char* lut256, const float* mean3, const float* std3, const float* blur_w,
                            float* scratch, float* out_img, long long* out_lab, hipStream_t stream);

/* ---- fp16 prediction path (csrc/half.hip): eval-mode forward with fp16 activations and weights.
   Activations are NHWC rows of IEEE fp16 (unsigned short bit patterns) with a pitch in elements; gfx950 only. ---- */
/* fp32 [Cout][Cin][R][S] -> fp16 [Cout][R][S][Cin], round to nearest even (BatchNorm is NOT folded in) */
int u2pl_half_weight_f16(const float* w, int Cout, int Cin, int R, int S, unsigned short* out, hipStream_t stream);
/* dense convolution, implicit GEMM on v_mfma_f32_32x32x16_f16 with fp32 accumulation.  x: pitch ldx >= Cin (a multiple
   of 8, base 16-byte aligned), Cin % 32 == 0; w from u2pl_half_weight_f16; any R x S, stride, pad, dil (Hout / Wout are
   checked against them).  Epilogue in fp32: v = acc * scale[c] + shift[c] (scale NULL: 1, shift NULL: 0), + res (fp16,
   pitch ldr, NULL: none), ReLU (relu != 0), then ONE rounding to fp16 into y (pitch ldy >= Cout: a channel slice of a
   concat buffer), or out_f32 != 0: y is float with pitch ldy and nothing is rounded.  A value with |v| > 65504 is stored
   as +-65504 and *sat (int32, device, zeroed by the caller; NULL: not counted) is incremented.  tile: 0 = the launcher
   chooses 64 or 128 pixel rows per block, 1 / 2 force one (tests). */
int u2pl_hconv2d_fwd_f16(const unsigned short* x, long ldx, const unsigned short* w, const float* scale,
                         const float* shift, const unsigned short* res, long ldr, void* y, long ldy, int N, int Hin,
                         int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil,
                         int relu, int out_f32, int tile, int* sat, hipStream_t stream);
/* direct form for a few input channels (the stem: Cin = 3): x is the fp32 NHWC image (u2pl_infer_input_u8_f32's
   layout), R * S * Cin * Cout <= 8192; same epilogue without a residual, fp16 output */
int u2pl_hconv2d_stem_f16(const float* x, long ldx, const unsigned short* w, const float* scale, const float* shift,
                          unsigned short* y, long ldy, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout,
                          int R, int S, int stride, int pad, int dil, int relu, int* sat, hipStream_t stream);
/* MaxPool2d(3, 2, 1, ceil_mode=True); C % 8 == 0, pitches multiples of 8, bases 16-byte aligned */
int u2pl_hmaxpool3s2_f16(const unsigned short* x, long ldx, int N, int H, int W, int C, int Ho, int Wo,
                         unsigned short* y, long ldy, hipStream_t stream);
/* y [N][C] = fp16(mean over the HW pixels of x [N][HW] rows), fp32 sums in a fixed order */
int u2pl_hgap_f16(const unsigned short* x, long ldx, int N, int HW, int C, unsigned short* y, hipStream_t stream);
/* bilinear, align_corners=True, [N][h][w] rows -> [N][H][W] rows with pitch ldy: ac_coord and the three-FMA expression
   of u2pl_bilinear_up_f32 on the widened taps, one rounding; C % 8 == 0, pitches multiples of 8, 16-byte bases */
int u2pl_hbilinear_f16(const unsigned short* x, long ldx, int N, int h, int w, int C, unsigned short* y, long ldy,
                       int H, int W, hipStream_t stream);

/* ---- more than 32 classes (reliability.hip, contrast_wide.hip) -----------------------------------------------------
 * The entry points above keep a pixel's multi-hot label in ONE 32-bit word (C <= 32).  These take 1 <= C <= 255 (label
 * value 255 is the ignore value; U2PL_EINVAL otherwise): class bits are WORD PLANES, u32 [W][P] with
 * W = u2pl_wide_words(C) = ceil(C / 32), plane g = classes 32 g .. 32 g + 31, P = pixels of the concatenated low-res
 * batch.  Counts are u32 [3][C] (kind 0 anchors, 1 low-valid, 2 negative keys), and the pixel lists live in ONE flat
 * int32 buffer, back to back in (kind, class) order, each in row-major pixel order; offsets int64 [3][C] = first element
 * of every list.  The caller reads counts back, allocates the flat buffer (sum of the counts) and then has the lists
 * written. */
int u2pl_wide_words(int C);
/* label_onehot (utils.py:50-59, slot-0 quirk) + masks + legacy-nearest down-sampling: train_semi.py:408-465; the forms
 * of u2pl_reliability_masks / u2pl_reliability_apply with lbits as planes [W][2B*h*w] */
int u2pl_reliability_masks_wide(const float* entropy, const unsigned* thr_lo_bits, const unsigned* thr_hi_bits,
                                const long long* label_l, const long long* label_u, int ignore, int B, int H, int W,
                                int h, int w, int negative_high_entropy, int C, float* low_mask, float* high_mask,
                                unsigned* lbits, hipStream_t stream);
int u2pl_reliability_apply_wide(const float* entropy, const unsigned* thr_bits, const long long* label_l,
                                const long long* label_u, int ignore, int B, int H, int W, int h, int w,
                                int negative_high_entropy, int C, long long* target_u, unsigned* nkept, float* low_mask,
                                float* high_mask, unsigned* lbits, hipStream_t stream);
/* (N,C,h,w) int64 multi-hot (the label_l / label_u arguments of compute_contra_memobank_loss, loss_helper.py:51-66)
 * <-> planes [W][N*h*w] */
int u2pl_pack_class_bits_wide(const long long* onehot, int N, int C, int h, int w, unsigned* bits, hipStream_t stream);
int u2pl_unpack_class_bits_wide(const unsigned* bits, int N, int C, int h, int w, long long* onehot, hipStream_t stream);
/* loss_helper.py:103-141: the masks of u2pl_contra_classify as planes (rank over the pixel's whole row of C
 * probabilities, ties towards the lower class index), then the list lengths (counts) and list offsets.  workspace:
 * u2pl_contra_wide_workspace_bytes(P, C) bytes, handed on to u2pl_compact_lists_wide.  A block owns
 * u2pl_contra_wide_block_pixels(C) pixels (256 up to C = 47, 128 up to 93, else 64). */
size_t u2pl_contra_wide_workspace_bytes(long P, int C);
int u2pl_contra_wide_block_pixels(int C);
/* 1: contiguous [pixel][C] probability rows are staged in LDS (C <= 183); 0: every thread reads its row from memory */
int u2pl_contra_wide_staged(int C);
int u2pl_contra_classify_wide(const float* prob, long sn, long sc, long sp, const unsigned* lbits, const float* low_mask,
                              const float* high_mask, int N2, int num_labeled, int C, int h, int w, float thr_p,
                              float thr_n, int low_rank, int high_rank, unsigned* abits, unsigned* lowbits,
                              unsigned* nbits, void* workspace, unsigned* counts, long long* offsets,
                              hipStream_t stream);
/* boolean-mask indexing order (loss_helper.py:115-116,119-123,142) for all three kinds into idx int32 [idx_len] */
int u2pl_compact_lists_wide(const unsigned* abits, const unsigned* lowbits, const unsigned* nbits, long P, int C,
                            const void* workspace, const long long* offsets, int* idx, long idx_len,
                            hipStream_t stream);
/* torch.mean(rep_teacher[low_valid], dim=0): loss_helper.py:119-123, ordered double-precision sums over the
 * low-valid lists; proto float [C][D], NaN rows for classes without members */
int u2pl_class_prototypes_wide(const float* rows, long ld, int D, const int* idx, const long long* offsets,
                               const unsigned* counts, int C, float* proto, hipStream_t stream);
/* dequeue_and_enqueue (utils.py:27-47) on the device-resident bank of u2pl_bank_init / u2pl_bank_enqueue_f32 (same
 * state layout): class c appends rows[idx[list_off_dev[c] + j]], j < counts_dev[c] */
int u2pl_bank_init_wide(long long* state, int C, const long long* caps_host, hipStream_t stream);
int u2pl_bank_enqueue_wide_f32(long long* state, float* storage, int D, const float* rows, long ld, const int* idx,
                               const long long* list_off_dev, const long long* row_start_dev,
                               const unsigned* counts_dev, int C, hipStream_t stream);

/* ---- lovasz.hip -------------------------------------- */
/* Segmented stable radix sort of (key, payload) uint32 pairs: segment s occupies elements [s * n, s * n + len_s) of keys /
 * vals, len_s = seg_len_dev[s] clamped to [0, n] (seg_len_dev == NULL: every segment holds n).  Ascending on the low `bits`
 * bits of the key (higher bits are carried along and ignored), equal keys keep their input order.  Least significant digit
 * first, 8-bit digits, u2pl_segsort_passes(bits) = ceil(bits / 8) passes of histogram -> scan -> scatter between the two
 * buffer pairs: after an even number of passes the result stands in keys / vals, after an odd number in keys_alt /
 * vals_alt; the other pair holds the previous pass.  Elements past len_s are neither read nor written.  A wave orders a tile
 * of u2pl_segsort_tile() elements; no block waits on another (the prefix over the tiles is a launch of its own), no atomics.
 * ws: u2pl_segsort_ws_bytes(nseg, n) bytes, contents on entry do not matter.
 * A null pointer, nseg outside [1, 65535], n outside [1, 2^31), bits outside [1, 32]: 1001 (ws_bytes and passes: 0). */
int u2pl_segsort_passes(int bits);
int u2pl_segsort_tile(void);
size_t u2pl_segsort_ws_bytes(int nseg, long n);
int u2pl_segsort_u32(unsigned* keys, unsigned* vals, unsigned* keys_alt, unsigned* vals_alt, void* ws, int nseg, long n,
                     const int* seg_len_dev, int bits, hipStream_t stream);
/* Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018, Algorithm 1 on the softmax errors) over the flattened batch:
 * logits [N][C][H][W], target int64 [N][H][W], P = N H W pixels, pixels with target == ignore take no part.
 *   m_i(c) = |[y_i == c] - softmax(z_i)[c]|; the valid pixels of class c sorted by m descending, ties in ascending pixel
 *   index; F_j = foreground among the first j, G = foreground of the class, I_j = G - F_j, U_j = G + (j - F_j);
 *   g_j = 1 / U_j (foreground), I_j / ((U_j - 1) U_j) (background, G > 0), [j == 1] (G == 0), formed in double;
 *   loss_c = sum_j m_j g_j, loss = mean of loss_c over the classes with G > 0 (present_only) or over all C classes.
 * Classes are processed in chunks of class_chunk (clamped to C; u2pl_lovasz_default_chunk() = 32, one chunk for Cityscapes);
 * for each chunk start c0 = 0, cap, 2 cap, ... call errors -> sort -> grad, then finish once, all with the same ws and
 * class_chunk.  ws: u2pl_lovasz_workspace_bytes(P, C, class_chunk) bytes, contents on entry do not matter.
 *   errors  keys (0x3F800000 - bits(m); 0x3FFFFFFF on ignored pixels) and payloads (pixel | foreground << 31) of the chunk
 *           [cc][P], the counts G[c] of its classes and the valid count
 *   sort    u2pl_segsort_u32 on those buffers, 30 bits; the sorted order stands where errors wrote
 *   grad    gplane[c][pixel] = g at the pixel's position (0 on ignored pixels and, with present_only, on absent classes) for
 *           the classes of the chunk; every slot written once; fp32 slabs of m g per (class, tile)
 *   finish  out3 = {loss, 1 / n_classes (0 when none), n_classes}; slabs added in double in a fixed order
 *   bwd     grad[n][c][q] = p_c (a_c - sum_k a_k p_k), a_c = -/+ gplane[c][i] out3[1] gout gmul (minus where c == y_i); 0 on
 *           ignored pixels.  gout_dev may be NULL (1).
 * No atomics, no host read, the same bits on every run.  plan (host only): out[20] = {chunks, classes per chunk, tile,
 * tiles per segment, errors blocks, count-reduction blocks, sort passes, sort / gradient grid.x, sort row-scan blocks,
 * gradient row-scan blocks, byte offsets in ws of keys, payloads, alternate keys, alternate payloads, sort workspace,
 * tile foreground counts, count partials, counts uint32 [C + 1] (G per class, then the valid count), slabs float
 * [C][tiles], total bytes}.
 * C outside [2, 255], P outside [1, 2^31), class_chunk < 1, a null required pointer, c0 not a chunk start: 1001 before any
 * HIP call (workspace_bytes: 0). */
size_t u2pl_lovasz_workspace_bytes(long P, int C, int class_chunk);
int u2pl_lovasz_default_chunk(void);
int u2pl_lovasz_plan(long P, int C, int class_chunk, long long* out);
int u2pl_lovasz_errors_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H, int W,
                           int c0, void* ws, int class_chunk, hipStream_t stream);
int u2pl_lovasz_sort(long P, int C, int c0, void* ws, int class_chunk, hipStream_t stream);
int u2pl_lovasz_grad_f32(long P, int C, int c0, int present_only, void* ws, int class_chunk, float* gplane,
                         hipStream_t stream);
int u2pl_lovasz_finish_f32(long P, int C, int present_only, const void* ws, int class_chunk, float* out3,
                           hipStream_t stream);
int u2pl_lovasz_bwd_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H, int W,
                        const float* gplane, const float* out3_dev, const float* gout_dev, float gmul, float* grad,
                        hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* U2PL_HIP_H */
