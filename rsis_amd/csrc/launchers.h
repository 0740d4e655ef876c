// Host functions that cross translation units of librsis_hip.so: the launchers the entry points of api.hip dispatch to.  api.hip and
// every file that defines one of them include this header, so the compiler checks each definition against the one declaration.
#pragma once
#include "common.h"
#include "../../include/rsis_hip.h"

// the conv kernels: rsis_launch_conv_X is defined in conv_X.hip (conv3x3_direct.hip: also the grouped launches; conv_blk.hip: the layout converters)
int rsis_launch_conv_igemm(ConvArgs& a, int ks, bool dgrad, int epi, int force_tile, hipStream_t st);
int rsis_launch_conv3x3_direct(ConvArgs& a, int epi, int force_variant, hipStream_t st);
int rsis_launch_convlstm_direct_group(ConvArgs* jobs, int n, const int* force_variant, hipStream_t st);
int rsis_launch_conv3x3_direct_group_plain(ConvArgs* jobs, int n, const int* force_variant, hipStream_t st);
int rsis_launch_conv_wino(const float* x, const void* U, const float* bias, const float* addend, float* y, int B, int C, int Cout, int H, int W, hipStream_t st,
                          int precise);
int rsis_launch_conv_wino_group(int n, const float* const* x, const void* const* U, float* const* y, float* const* y1, const int* B, const int* C, const int* Cout,
                                const int* C0, const int* H, const int* W, hipStream_t st);
int rsis_launch_conv_bf16(ConvArgs& a, int ks, int epi, int force_variant, hipStream_t st);
int rsis_launch_conv_blk(ConvArgs& a, int ks, int variant, hipStream_t st);
int rsis_l_blk_from_nchw(const float* x, void* y, int B, int C, int HW, hipStream_t st);
int rsis_l_blk_to_nchw(const void* x, float* y, int B, int C, int HW, hipStream_t st);
int rsis_launch_conv_blk_dec(BlkConvJob* jobs, int n, int epi, const int* force_variant, hipStream_t st);
int rsis_launch_conv_wgrad(WgradArgs& a, int ks, hipStream_t st);
bool rsis_wgrad_bf16_supported(const WgradArgs& w, int ks);
int rsis_wgrad_staged_limbs(const WgradArgs& w, int ks);      // fp32 job: 1 = the staged limb kernels take it, 0 = not, -1 = forced and refused
int rsis_launch_conv_wgrad_bf16_group(const WgradArgs* w, int n, int ks, hipStream_t st);
int rsis_launch_conv_wgrad_bf16(const WgradArgs& w, int ks, hipStream_t st);
int rsis_launch_conv_wgrad_tiled_group(const WgradArgs* w, int n, int ks, hipStream_t st);
int rsis_launch_conv_wgrad_tiled(const WgradArgs& w, int ks, hipStream_t st);
bool rsis_wgrad_tiled_supported(const WgradArgs& w, int ks);
// conv_c1.hip, upconv_out.hip: conv_out (one output channel), alone and fused with the x2 upsample
bool rsis_c1_supported(int Cin);
int rsis_l_c1_fwd(const float* x, const float* wp, int ldw, const float* bias, float* y, int B, int Cin, int H, int W, int seqT, hipStream_t st);
int rsis_l_c1_dgrad(const float* dy, const float* wd, int ldw, float* dx, int B, int Cin, int H, int W, int seqT, hipStream_t st);
int rsis_l_c1_wgrad(const float* dy, const float* x, float* dw, float* db, int B, int Cin, int H, int W, int seqT, hipStream_t st);
bool rsis_upconv_supported(int C, int Hs, int Ws, int Ho, int Wo);
int rsis_upconv_bwd_blocks(int T, int B, int Hs, int Ws);
int rsis_l_upconv_fwd(const void* h, int h_blk, const float* w, const float* bias, float* out, int T, int B, int Hs, int Ws, int Ho, int Wo, hipStream_t st);
int rsis_l_upconv_bwd(const float* dout, const void* h, int h_blk, const float* w, void* dh, float* dW, float* db, const float* dside, const int* arg,
                      float* partial, int T, int B, int Hs, int Ws, int Ho, int Wo, hipStream_t st);
// pack.hip (PackMode: common.h)
int rsis_l_pack_batch(const rsis_pack_job* jobs, int njobs, int total_blocks, hipStream_t st);
int rsis_l_pack_blocks(PackMode mode, int krows, int ldw, int ks);
int rsis_l_pack(PackMode mode, const float* W, void* out, int Cout, int Ctot, int ks, int nseg, const int* Cseg, const int* Coff, int ldw, int krows, int hid,
                hipStream_t st);
// pointwise.hip, optim.hip
int rsis_l_lstm_bwd(const float* dh, const float* dh2, const float* dc_next, const float* act, const float* c_prev, const float* c, float* da, float* dc_prev,
                    float* da_sum, int B, int hid, int HW, hipStream_t st);
int rsis_l_lstm_bwd_group(const void* const* ptrs, const int* dims, int n, hipStream_t st);
// (scale: [BC] factors of the planes of the result, null = none -- the kernels without the argument)
int rsis_l_upsample_fwd(const float* x, float* y, long BC, int Hi, int Wi, int Ho, int Wo, const float* scale, hipStream_t st,
                        const float* mul = nullptr);
int rsis_l_upsample_mul_bwd_prep(float* dy, const float* x, const float* m, float* dm, long BC, int Hi, int Wi, int Ho, int Wo, int accumulate,
                                 hipStream_t st);
int rsis_l_upsample_bwd(const float* dy, float* dx, long BC, int Hi, int Wi, int Ho, int Wo, const float* pool_g, const int* pool_arg, const float* scale,
                        hipStream_t st);
int rsis_l_scale_planes(const float* x, const float* scale, float* y, long BC, int HW, hipStream_t st);
int rsis_l_gmax_fwd(const float* x, float* y, int* arg, long BC, int HW, hipStream_t st);
int rsis_l_gmax_bwd(const float* dy, const int* arg, float* dx, long BC, int HW, hipStream_t st);
int rsis_l_bn_fwd(const float* x, const float* res, float* y, unsigned char* mask, double* stats, const float* gamma, const float* beta, float* run_mean,
                  float* run_var, float* save_mean, float* save_rstd, int B, int C, int HW, float eps, float momentum, int relu, int train_flags, hipStream_t st);
int rsis_l_bn_bwd(const float* dy, const float* x, const float* y, const unsigned char* mask, const float* mean, const float* rstd, const float* gamma,
                  double* stats, float* dx, float* dres, float* dgamma, float* dbeta, int B, int C, int HW, int relu_flags, float eval_eps, hipStream_t st);
int rsis_l_gmax_bwd_add(const float* dy, const int* arg, float* dx, long BC, int HW, const float* scale, hipStream_t st);
int rsis_l_subsample(const float* x, float* y, long BC, int H, int W, int Ho, int Wo, int s, hipStream_t st);
int rsis_l_maxpool_fwd(const float* x, float* y, unsigned char* arg, long BC, int H, int W, int Ho, int Wo, hipStream_t st);
int rsis_l_maxpool_bwd(const float* dy, const unsigned char* arg, float* dx, long BC, int H, int W, int Ho, int Wo, int accumulate, hipStream_t st);
int rsis_l_sum_leading(const float* x, float* y, int T, long n, hipStream_t st);
int rsis_l_channel_sum(const float* dy, float* db, int B, int C, int HW, int hid, hipStream_t st);
int rsis_l_adam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float wd, int step, float gscale, const int* step_dev,
                hipStream_t st);
int rsis_l_assign(const float* scores, long long* perm, int B, int G, int T, hipStream_t st);
int rsis_l_flat_rule(int rule, float* p, const float* g, float* s, long n, float lr, float c0, float c1, float wd, float gscale, hipStream_t st);
// blk_norm.hip, blk_dec.hip: channel-blocked bf16 tensors
long rsis_l_blk_bn_scratch(int C);
int rsis_l_blk_bn_fwd(const void* x, const void* res, void* y, double* scratch, const float* gamma, const float* beta, float* run_mean, float* run_var,
                      float* save_mean, float* save_rstd, int B, int C, int HW, float eps, float momentum, int relu, int train, hipStream_t st);
int rsis_l_blk_bn_bwd(const void* dy, const void* x, const void* y, double* scratch, const float* gamma, const float* beta, const float* save_mean,
                      const float* save_rstd, void* dx, void* dres, float* dgamma, float* dbeta, int accumulate, int B, int C, int HW, int relu, hipStream_t st);
int rsis_l_blk_subsample(const void* x, void* y, long BCb, int H, int W, int Ho, int Wo, int stride, hipStream_t st);
int rsis_l_blk_upscatter(const void* dy, void* dx, long BCb, int H, int W, int Ho, int Wo, int stride, hipStream_t st);
int rsis_l_blk_upsample_fwd(const BlkResizeJob* jobs, int n, hipStream_t st);
int rsis_l_blk_upsample_bwd(const BlkResizeJob* jobs, int n, hipStream_t st);
int rsis_l_blk_upsample_fwd_scaled(const BlkResizeScaledJob* jobs, int n, hipStream_t st);
int rsis_l_blk_upsample_bwd_scaled(const BlkResizeScaledJob* jobs, int n, hipStream_t st);
int rsis_l_blk_upsample_mul_fwd(const BlkResizeMulJob* jobs, int n, hipStream_t st);
int rsis_l_blk_upsample_mul_bwd_prep(const BlkMulPrepJob* jobs, int n, hipStream_t st);
int rsis_l_blk_lstm_bwd(const BlkLstmBwdJob* jobs, int n, hipStream_t st);
int rsis_l_blk_sum_leading(const void* x, void* y, int T, long n, hipStream_t st);
int rsis_l_blk_channel_sum(const void* dy, float* db, int B, int C, int HW, int hid, hipStream_t st);
int rsis_l_blk_c1_fwd(const void* x, const float* w, const float* bias, float* y, int T, int B, int H, int W, hipStream_t st);
int rsis_l_blk_c1_dgrad(const float* dy, const float* w, void* dx, int T, int B, int H, int W, hipStream_t st);
int rsis_l_blk_c1_wgrad(const float* dy, const void* x, float* dw, float* db, int T, int B, int H, int W, hipStream_t st);
// dropout.hip: the decoder's dropout scales (include/rsis_hip.h: rsis_dropout_scales) and the head masks
int rsis_l_dropout_scales(unsigned* state, float* s2, float* mc, float* ms, long n, float p2, float pc, float ps, hipStream_t st);
int rsis_l_dropout_heads_mask(float* side, const float* s2, const float* mc, const float* ms, float* side_c, float* side_s, long n, hipStream_t st);
int rsis_l_dropout_heads_mask_bwd(const float* dc, const float* ds, const float* mc, const float* ms, float* dside, long n, hipStream_t st);
// losses.hip (the default arguments of rsis_l_heads_fwd stand here, on the declaration, only)
int rsis_l_softiou_sums(const float* logits, const float* y, float* S, int B, int T, int G, long N, hipStream_t st);
int rsis_l_softiou_bwd(const float* logits, const float* y, const long long* perm, int perm_ld, const float* ca, const float* cb, float* dlogits, int B, int T,
                       int G, long N, hipStream_t st);
// (ignore null = the plain launches above)
int rsis_l_softiou_sums_ignore(const float* logits, const float* y, const unsigned char* ignore, float* S, int B, int T, int G, long N, hipStream_t st);
int rsis_l_softiou_bwd_ignore(const float* logits, const float* y, const unsigned char* ignore, const long long* perm, int perm_ld, const float* ca,
                              const float* cb, float* dlogits, int B, int T, int G, long N, hipStream_t st);
int rsis_l_heads_fwd(const float* const* side, const int* C, int n, int B, const float* Wc, const float* bc, int ncls, const float* Ws, const float* bs,
                     float* probs, float* stop, hipStream_t st, const unsigned long long* const* keys = nullptr, float* const* side_out = nullptr,
                     int* const* arg_out = nullptr);
int rsis_l_heads_bwd(const float* const* side, const int* C, int n, int B, const float* Wc, int ncls, const float* Ws, const float* probs, const float* dprobs,
                     const float* dstop, float* const* dside, float* dWc, float* dbc, float* dWs, float* dbs, hipStream_t st);
int rsis_l_heads_wide_fwd(const float* const* side, const int* C, int n, int rows, const float* Wc, const float* bc, int ncls, const float* Ws,
                          const float* bs, float* probs, float* stop, hipStream_t st, const unsigned long long* const* keys = nullptr,
                          float* const* side_out = nullptr, int* const* arg_out = nullptr);
int rsis_l_heads_wide_bwd(const float* const* side, const int* C, int n, int rows, const float* Wc, int ncls, const float* Ws, const float* probs,
                          const float* dprobs, const float* dstop, float* const* dside, float* dWc, float* dbc, float* dWs, float* dbs, float* scratch,
                          long scratch_floats, hipStream_t st);
int rsis_l_loss_tail(const float* probs, const long long* y_class, const float* stop, const float* siou, const float* sw_mask, const float* sw_class,
                     const float* cls_w, int n, int C, float bw, float w_iou, float w_cls, float w_stop, float* out, float* dprobs, float* dstop, float* dsiou,
                     const float* gout, hipStream_t st);
// the data layer: augment.hip, targets.hip, instmaps.hip, pascalprep.hip
int rsis_l_affine_nearest(const float* x, float* y, const float* mat, int N, int C, int H, int W, int mat_stride, hipStream_t st);
long rsis_l_targets_work_ints(int B);
int rsis_l_targets_from_maps(const int* ins, const int* seg, int B, int H, int W, int T, float* y_mask, long long* y_class, float* sw_mask, float* sw_class,
                             int* work, hipStream_t st);
long rsis_l_instance_maps_work_ints(int B);
int rsis_l_instance_maps(const int* raw, const int* class_of_label, int n_labels, int B, int H, int W, int* ins, int* seg, int* work, hipStream_t st);
int rsis_l_palette_to_ids(const unsigned char* rgb, long npix, const unsigned char* table, int ntab, unsigned char* ids, hipStream_t st);
int rsis_l_idmap_rle_encode(const unsigned char* idmap, int h, int w, const int* ids, int k, unsigned int* counts, int cap, int* nruns, hipStream_t st);
// evaluation: maskpost.hip, overlay.hip, maskeval.hip, labeleval.hip, insteval.hip
int rsis_l_mask_resize_threshold(const float* prob, int n, int Hm, int Wm, const unsigned char* ignore, float th, unsigned char* seg, unsigned char* raw,
                                 unsigned int* area, int h, int w, hipStream_t st);
int rsis_l_rle_encode(const unsigned char* masks, int n, long len, unsigned int* counts, int cap, int* nruns, hipStream_t st);
int rsis_l_rle_to_string(const unsigned int* counts, int m, char* out, int cap);
int rsis_l_largest_component(const unsigned char* mask, unsigned char* out, int* labels, int* counts, int* best, int n, int h, int w, hipStream_t st);
int rsis_l_overlay_moments(const unsigned char* masks, int n, const int* order, int k, int h, int w, unsigned long long* moments, hipStream_t st);
int rsis_l_overlay_masks(const unsigned char* image, const unsigned char* masks, int n, const int* order, const unsigned char* colors, int k, float alpha,
                         unsigned char* out, int h, int w, hipStream_t st);
int rsis_l_mask_pack_bits(const unsigned char* masks, int n, long len, unsigned long long* bits, long stride, unsigned int* area, hipStream_t st);
int rsis_l_rle_to_bits(const unsigned int* counts, long counts_len, const long long* desc, int n, unsigned int* ends, unsigned long long* bits, long bits_len,
                       unsigned int* area, hipStream_t st);
int rsis_l_poly_to_bits(const double* xy, long nverts, const long long* parts, long nparts, const long long* recs, int n, unsigned long long* scratch,
                        unsigned long long* bits, long bits_len, unsigned int* area, hipStream_t st);
int rsis_l_paint_ignore_map(const unsigned long long* bits, long bits_len, long nrec, const long long* crecs, const long long* imgs, int B, int max_recs,
                            const int* src_y, const int* src_x, int Ho, int Wo, const int* ins, unsigned char* ign, hipStream_t st);
int rsis_l_paint_instance_maps(const unsigned long long* bits, long bits_len, const unsigned int* area, long nrec, const long long* recs,
                               const long long* imgs, int B, int max_recs, const int* src_y, const int* src_x, int Ho, int Wo, int* ins, int* seg,
                               hipStream_t st);
long rsis_l_mask_intersect_blocks(long D, long G, long stride);
int rsis_l_mask_intersect_batch(const unsigned long long* bits, long bits_len, const long long* jobs, int njobs, int total_blocks, unsigned int* inter,
                                long inter_len, hipStream_t st);
int rsis_l_coco_iou_batch(const long long* cells, int ncells, const unsigned int* inter, long inter_len, const int* dt_row, const unsigned int* dt_marea, long ndt,
                          const int* gt_col, const unsigned int* gt_marea, const int* gt_crowd, long ngt, double* ious, long ious_len, hipStream_t st);
int rsis_l_coco_match_batch(const long long* cells, int ncells, const double* ious, long ious_len, const int* gperm, const int* gflag, long ngt,
                            const double* dt_area, long ndt, const double* arng, int nrng, const double* thrs, int T, int* dtm, int* dti, long dt_out_len, int* gtm,
                            long gt_out_len, hipStream_t st);
int rsis_l_rle_from_string(const char* s, unsigned int* counts, int cap);
long rsis_l_label_contingency_blocks(long npix);
int rsis_l_label_contingency_batch(const unsigned char* pool, long pool_len, const long long* jobs, int njobs, int total_blocks, unsigned int* counts,
                                   long counts_len, hipStream_t st);
int rsis_l_label_scores_batch(const unsigned int* counts, long counts_len, const long long* jobs, int njobs, double* scores, hipStream_t st);
long rsis_l_inst_overlap_blocks(long npix, long P);
int rsis_l_inst_presence_batch(const unsigned char* pool, long pool_len, const long long* jobs, int njobs, int total_blocks, unsigned char* flags, long flags_len,
                               hipStream_t st);
int rsis_l_inst_overlap_batch(const unsigned char* pool, long pool_len, const long long* jobs, int njobs, int total_blocks, const unsigned short* lut, long lut_len,
                              const unsigned long long* bits, long bits_len, unsigned int* counts, long counts_len, hipStream_t st);
