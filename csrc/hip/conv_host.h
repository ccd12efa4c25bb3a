// Host-side launchers of the convolution / wgrad kernels that one .hip file defines and another
// calls (internal: C++ linkage, not part of the exported C ABI in rag_api.h).
#pragma once
#include "common.h"
#include "wgrad_part.h"

// A deferred wgrad partial-slab reduction waiting in a caller-owned handle
// (ops.PendingReduction; rag_wgrad_pending_* in conv.hip).
struct PendingRed {
  int valid;
  hipStream_t stream;
  rag::WgradRed r;
  unsigned* dticket;  // the handle's [2] device claim counters (rag_wgrad_pending_init)
};

// One forward / dgrad convolution launch as conv.hip hands it to the kernel files.
struct ConvLaunch {
  const bf16* x;
  const bf16* w;
  const float* bias;
  bf16* y;
  const bf16* mask;  // dgrad ReLU mask (halo HM) or null
  const bf16* res;   // residual (laid out like y) or null
  int M, S, WI, shift, WO, HO, CIN, COUTP, YC, KS, relu, HM;
  long total_rows;
  hipStream_t stream;
  int cin_real;              // real input channels of the padded CIN (0: all of them)
  const rag::WgradRed* red;  // a pending reduction riding along the launch, or null
  const float* bnc;          // BN prologue coefficients (conv_tap_pp_kernel BNP) or null
  const float* mcoef;        // BN mask coefficients (dgrad form) or null
  float* spart;              // BN column statistics partials or null
  const float* smean;        // BN mean for the backward statistics or null
};

// conv_tap.hip: true if one of its kernels took the launch (red rides along then).
bool rag_conv_tap_launch(const ConvLaunch& c);
bool rag_conv_tap_bn_ok(int M, int S, int WI, int shift, int CIN, int COUTP, int KS);
// conv_fwd.hip: true if the pipelined kernel took the launch (no BN forms, no riding reduction).
bool rag_conv_pipe_launch(const ConvLaunch& c);

// conv_wino.hip
int rag_conv_wino_launch(const void* X, const void* W, const float* bias, void* Y,
                         const void* mask, int B, int S, int KIN, int NOUT, int HO, int YC,
                         int relu, int HM, hipStream_t stream, const rag::WgradRed* red, int half);
int rag_conv_wino_bn_launch(const void* X, const void* W, const float* bias, void* Y,
                            const void* mask, const void* res, int B, int S, int KIN, int NOUT,
                            int HO, int YC, int relu, int HM, hipStream_t stream,
                            const rag::WgradRed* red, const float* coef, const float* mcoef,
                            float* spart, const float* smean);

// wgrad.hip
int rag_launch_wgrad_taps(const bf16* G, const bf16* X, float* part, float* bpart, int R, int WP,
                          int GC, int CIN, int spc, int COUTP, int CINP, int KS, int RG,
                          int nchunks, hipStream_t stream);
bool rag_wgrad_taps_fits(int WP, int KS, int RG);
int rag_wgrad_taps_target_blocks();

// wgrad_slab.hip
bool rag_wgrad_slab_ok(int S, int H, int HG, int GC, int COUTP, int CINP, int KS);
int rag_wgrad_slab_nchunks(int R, int CINP, int* spc, int KS, int pair5);
bool rag_wgrad_slab_bf16();
rag::WgradRed rag_wgrad_slab_red(const void* part, const float* bpart, float* dW, float* db,
                                 int nchunks, int CINP, int COUTP, int COUT, int CIN,
                                 int accumulate, int KS, int pair5);
int rag_launch_wgrad_slab_reduce(const rag::WgradRed& r, hipStream_t stream);
int rag_launch_wgrad_slab(const bf16* G, const bf16* X, float* part, float* bpart, int R, int WP,
                          int GC, int CIN, int spc, int CINP, int nchunks, hipStream_t stream,
                          const float* xcoef, int S, int KS, int COUTP, int pair5,
                          unsigned* ticket_reset);
