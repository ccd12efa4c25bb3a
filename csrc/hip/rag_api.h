// The exported C ABI of _hipkernels.so: every RAG_API function, declared once. Each .hip that
// defines one includes this header, so the compiler rejects a definition that disagrees, and
// tests/test_native_symbols.py compares these prototypes with the ctypes table
// (rocalphago_amd/ops/_abi.py). Keep it flat: one `RAG_API <ret> rag_name(<args>);` each, no
// macros or default arguments. Optional pointer arguments are null, optional ints 0.
#pragma once
#include "common.h"

// ---- conv.hip
RAG_API size_t rag_wgrad_pending_bytes();
RAG_API int rag_wgrad_pending_init(void* h);
RAG_API int rag_wgrad_pending_free(void* h);
RAG_API int rag_wgrad_flush(hipStream_t stream, void* pending);
RAG_API int rag_conv_bn_fusable(int B, int S, int HI, int CIN, int COUTP, int KS);
RAG_API int rag_conv_bn_stat_blocks(int B, int S, int COUTP);
RAG_API int rag_conv_igemm(const void* X, const void* W, const float* bias, void* Y,
                           const void* mask, const void* resid, int B, int S, int HI, int HO,
                           int CIN, int COUTP, int YC, int KS, int relu, int HM,
                           hipStream_t stream, void* pending, int cin_real, const float* bnc,
                           const float* mcoef, float* spart, const float* smean);
RAG_API int rag_conv_wino(const void* X, const void* W, const float* bias, void* Y,
                          const void* mask, int B, int S, int KIN, int NOUT, int HO, int YC,
                          int relu, int HM, hipStream_t stream, void* pending, int half);
RAG_API int rag_conv_wino_bn(const void* X, const void* W, const float* bias, void* Y,
                             const void* mask, const void* resid, int B, int S, int KIN, int NOUT,
                             int HO, int YC, int relu, int HM, hipStream_t stream, void* pending,
                             const float* coef, const float* mcoef, float* spart,
                             const float* smean);
RAG_API size_t rag_conv_wgrad_workspace(int B, int S, int COUTP, int CINP, int KS, int* nchunks);
RAG_API int rag_conv_wgrad(const void* G, const void* X, float* dW, float* db, float* work,
                           int B, int S, int HI, int HG, int GC, int COUT, int COUTP, int CIN,
                           int CINP, int KS, int accumulate, hipStream_t stream, void* pending,
                           const float* xcoef);
RAG_API int rag_pack_weights(const float* W, void* Wf, void* Wb, int COUT, int CIN, int KS,
                             int COUTP, int CINP, hipStream_t stream);
RAG_API int rag_pack_trunk(const int64_t* table, int nrows, int nfull, int64_t total,
                           hipStream_t stream, int64_t goff, float lr, float wd, int sgd_on);
RAG_API int rag_pack_input_u8(const uint8_t* F, const int64_t* index, const int* tf, void* X,
                              int B, int NF, int FS, int S, int H, int CP, hipStream_t stream);
RAG_API int rag_pack_input_f32(const float* F, const int64_t* index, const int* tf, void* X,
                               int B, int NF, int FS, int S, int H, int CP, hipStream_t stream);
RAG_API int rag_pack_input_bits(const uint64_t* Fb, const int64_t* index, const int* tf, void* X,
                                int B, int NF, int S, int H, int CP, hipStream_t stream);
RAG_API int rag_unpack(const void* X, float* out, int B, int C, int S, int H, int CP,
                       hipStream_t stream);
RAG_API int rag_pack_nchw(const float* in, void* X, int B, int C, int S, int H, int CP,
                          hipStream_t stream);

// ---- conv_wino.hip
RAG_API int rag_conv_wino_ok(int S, int HI, int KIN, int NOUT, int KS);
RAG_API int rag_conv_wino_mode(int B, int S, int KIN, int NOUT);
RAG_API int rag_conv_wino_bn_ok(int B, int S, int KIN, int NOUT);
RAG_API int rag_conv_wino_bn_ch(const void* X, const void* W, const float* bias, void* Y,
                                const void* resid, int B, int S, int KIN, int NOUT, int HO, int YC,
                                int relu, hipStream_t stream, const float* coef, float* spart);
RAG_API int rag_conv_wino_chain(const int64_t* table, int L, int B, int S, hipStream_t stream,
                                int any_batch);
RAG_API int rag_wino_pack(const int64_t* table, int nlayers, int max_tiles, hipStream_t stream,
                          int64_t goff, float lr, float wd, int sgd_on);
RAG_API int rag_pack_step(const int64_t* wtable, int nwino, const int64_t* ttable, int nrows,
                          int nfull, int max_taps, int width, hipStream_t stream, int64_t goff,
                          float lr, float wd, int sgd_on, float* flat, int64_t a0, int64_t n0,
                          int64_t a1, int64_t n1);

// ---- conv_tap.hip, wgrad_slab.hip (A/B setters the tests drive; each returns the previous
// setting)
RAG_API int rag_conv_tap_mode(int mode);
RAG_API int rag_wgrad_slab_map(int m);
RAG_API int rag_wgrad_slab_part_bf16(int on);
// the slab weight gradient's row chunking: chunks (blocks per c-tile), *spc 64-row stages each
RAG_API int rag_wgrad_slab_chunks(int R, int CINP, int KS, int pair5, int* spc);

// ---- head.hip, value_bwd.hip
RAG_API int rag_pass_grads(const float* zout, const float* dpass, float* dW, float* db, int B,
                           int P, hipStream_t stream);
RAG_API int rag_policy_head_fwd(const void* H, const float* w, const float* b0,
                                const float* pbias, const float* pass_w, const float* pass_b,
                                float* probs, const int64_t* labels, const float* sweight,
                                float* loss, float* dz, float* hit, float* zout, float* dpass,
                                float* acc, float* dzsum, int B, int S, int KP, int K, int mode,
                                float gscale, hipStream_t stream);
RAG_API int rag_policy_head_soft(const void* H, const float* w, const float* b0,
                                 const float* pbias, const float* pass_w, const float* pass_b,
                                 float* probs, const float* targets, const float* sweight,
                                 float* loss, float* dz, float* hit, float* zout, float* dpass,
                                 float* dzsum, int B, int S, int KP, int K, float gscale,
                                 hipStream_t stream);
RAG_API int rag_head_bwd(const void* H, const float* w, const float* dz, void* dH, float* dw,
                         float* db0, float* dpbias, float* work, int B, int S, int KP, int K,
                         int relu_mask, const float* mloss, const float* mhit, float* acc,
                         const float* dzsum, hipStream_t stream);
RAG_API size_t rag_head_bwd_workspace(int B, int S, int KP);
RAG_API int rag_policy_head_dual(const void* H, const float* w, const float* b0,
                                 const float* pbias, const float* wv, const float* b0v,
                                 float* probs, float* zv, const int64_t* labels,
                                 const float* targets, const float* sweight, float* loss,
                                 float* dz, float* hit, float* dzsum, int B, int S, int KP, int K,
                                 int mode, float gscale, hipStream_t stream);
RAG_API int rag_head_bwd2(const void* H, const float* wp, const float* wv, const float* dzp,
                          const float* dzv, void* dH, float* dwp, float* dwv, float* db0p,
                          float* db0v, float* dpbias, float* work, int B, int S, int KP, int K,
                          int relu_mask, const float* mloss, const float* mhit, float* acc,
                          const float* dzsum, hipStream_t stream);
RAG_API size_t rag_head_bwd2_workspace(int B, int S, int KP);
RAG_API int rag_policy_head_dual_relu(const void* H, const float* w, const float* b0,
                                      const float* pbias, const float* wv, const float* b0v,
                                      float* probs, float* zv, const int64_t* labels,
                                      const float* targets, const float* sweight, float* loss,
                                      float* dz, float* hit, float* dzsum, int B, int S, int KP,
                                      int K, int mode, float gscale, hipStream_t stream);
RAG_API int rag_head_bwd2_relu(const void* H, const float* wp, const float* wv, const float* dzp,
                               const float* dzv, void* dH, float* dwp, float* dwv, float* db0p,
                               float* db0v, float* dpbias, float* work, int B, int S, int KP,
                               int K, const float* mloss, const float* mhit, float* acc,
                               const float* dzsum, hipStream_t stream);
RAG_API int rag_head_linear(const void* H, const float* w, const float* b0, float* z, int B,
                            int S, int KP, int K, hipStream_t stream);
RAG_API size_t rag_value_mlp_workspace(int B, int H);
RAG_API int rag_value_mlp_fwd(const float* z, const float* W1, const float* b1, const float* W2,
                              const float* b2, float* out, float* work, float* hout, int B,
                              int P, int H, int act, hipStream_t stream);
RAG_API size_t rag_value_mlp_bwd_workspace(int B, int H);
RAG_API int rag_value_mlp_bwd(const float* z, const float* W1, const float* W2, const float* b2,
                              const float* hpre, const float* part, const float* y,
                              const float* sw, float* work, float* loss, float* vout, float* dW1,
                              float* db1, float* dW2, float* db2, float* dz, int B, int P, int H,
                              int act, hipStream_t stream);

// ---- batch.hip, optim.hip, sample.hip
RAG_API int rag_sl_batch(const int64_t* index, const int64_t* labels, const int64_t* tf_table,
                         int P, const int* sym, int nsym, unsigned seed, unsigned step,
                         int* tf_out, int64_t* lab_out, int B, hipStream_t stream);
RAG_API int rag_sl_batch_soft(const int64_t* index, const uint16_t* visits, int CD,
                              const int64_t* tf_table, int P, const int* sym, int nsym,
                              unsigned seed, unsigned step, int* tf_out, float* targets_out,
                              int C, int B, hipStream_t stream);
RAG_API int rag_value_batch(const int64_t* index, const float* values, const int* sym, int nsym,
                            unsigned seed, unsigned step, int* tf_out, float* y_out, int B,
                            hipStream_t stream);
RAG_API int rag_sgd(float* p, const float* g, float* v, int64_t n, float lr, float momentum,
                    float wd, int nesterov, hipStream_t stream);
RAG_API int rag_sample_moves(const float* probs, const uint8_t* mask, int ms,
                             const uint8_t* greedy, int B, int P, float beta, uint64_t seed,
                             const uint64_t* seed_dev, int* moves, hipStream_t stream);

// ---- bn.hip
RAG_API int rag_bn_workspace(int B, int S);
RAG_API int rag_bn_train_fwd(const void* X, int hx, int B, int S, int C, int CP,
                             const float* gamma, const float* beta, float* rmean, float* rvar,
                             float eps, float momentum, float* stats, float* coef, float* work,
                             hipStream_t stream);
RAG_API int rag_bn_infer_coef(const float* gamma, const float* beta, float* rmean, float* rvar,
                              float eps, int S, float* coef, hipStream_t stream);
RAG_API int rag_bn_bwd_coef(const void* X, int hx, const void* DY, int hd, int B, int S, int C,
                            int CP, const float* gamma, const float* stats, float* dgamma,
                            float* dbeta, float* coef, float* work, hipStream_t stream);
RAG_API int rag_bn_finalize_fwd(const float* part, int nblk, int B, int S, int C,
                                const float* gamma, const float* beta, float* rmean, float* rvar,
                                float eps, float momentum, float* stats, float* coef,
                                hipStream_t stream);
RAG_API int rag_bn_finalize_bwd(const float* part, int nblk, int B, int S, int C,
                                const float* gamma, const float* stats, float* dgamma,
                                float* dbeta, float* coef, hipStream_t stream);
RAG_API int rag_bn_apply(const void* X, int hx, const void* DY, int hd, const void* RES, int hr,
                         void* O, int ho, const float* coef, int relu, int B, int S, int C, int CP,
                         hipStream_t stream);
RAG_API int rag_bn_apply_bwd_part(const float* part, int nblk, const float* gamma,
                                  const float* stats, float* dgamma, float* dbeta, const void* X,
                                  int hx, const void* DY, int hd, const void* RES, int hr, void* O,
                                  int ho, int B, int S, int C, int CP, hipStream_t stream);
// channel form (axis=1): one statistic per channel, CP slots of which the first C are real
RAG_API int rag_bn_ch_workspace(int B, int S, int CP);
RAG_API int rag_bn_ch_train_fwd(const void* X, int hx, int B, int S, int C, int CP,
                                const float* gamma, const float* beta, float* rmean, float* rvar,
                                float eps, float momentum, float* stats, float* coef, float* work,
                                hipStream_t stream);
RAG_API int rag_bn_ch_finalize_fwd(const float* part, int nblk, int B, int S, int C, int CP,
                                   const float* gamma, const float* beta, float* rmean,
                                   float* rvar, float eps, float momentum, float* stats,
                                   float* coef, hipStream_t stream);
RAG_API int rag_bn_ch_infer_coef(const float* gamma, const float* beta, float* rmean, float* rvar,
                                 float eps, int C, int CP, float* coef, hipStream_t stream);
RAG_API int rag_bn_ch_bwd_coef(const void* X, int hx, const void* DY, int hd, int B, int S, int C,
                               int CP, const float* gamma, const float* stats, float* dgamma,
                               float* dbeta, float* coef, float* work, hipStream_t stream);
RAG_API int rag_bn_ch_apply(const void* X, int hx, const void* DY, int hd, const void* RES, int hr,
                            void* O, int ho, const float* coef, int relu, int B, int S, int C,
                            int CP, hipStream_t stream);

// ---- features.hip, ladder.hip, rollout.hip
RAG_API int rag_features(const void* colors, const void* ages, const int32_t* meta,
                         const uint8_t* extra_illegal, const uint8_t* ladders, int n_pos, int S,
                         const int* fids, int nf, int F, uint8_t* out, uint8_t* sens,
                         hipStream_t stream);
RAG_API size_t rag_ladder_workspace(int n_pos, int S);
RAG_API int rag_ladders(const void* colors, const int32_t* meta, int n_pos, int S, void* work,
                        uint8_t* out, hipStream_t stream);
RAG_API long rag_rollout_park_bytes(int S);
RAG_API int rag_rollouts(const void* colors, const int32_t* meta, int n_pos, int R, int S,
                         float komi, int limit, const float* w, const float* pattern,
                         unsigned seed, void* winner, void* length, float* dbg_logits,
                         hipStream_t stream, void* park, int slice);
