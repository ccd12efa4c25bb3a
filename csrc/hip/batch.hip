// Per-step SL batch preparation in one launch: for each of the B sampled rows a
// random dihedral transform (one of the trainer's allowed symmetries) and the transformed target
// index. Replaces the random draw, the symmetry lookup and the two label gathers (four small
// library kernels per step).
#include "common.h"
#include "rag_api.h"

namespace {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// tf_out[i] = sym[h(seed, step, i) % nsym]; lab_out[i] = tf_table[tf_out[i]][labels[index[i]]]
__global__ void sl_batch_kernel(const int64_t* __restrict__ index,
                                const int64_t* __restrict__ labels,
                                const int64_t* __restrict__ tf_table, int P,
                                const int* __restrict__ sym, int nsym, uint32_t seed,
                                uint32_t step, int* __restrict__ tf_out,
                                int64_t* __restrict__ lab_out, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const uint32_t h = mix32(seed ^ mix32(step * 0x9E3779B9u + (uint32_t)i * 0x85EBCA6Bu + 1u));
  const int t = sym[h % (uint32_t)nsym];
  tf_out[i] = t;
  lab_out[i] = tf_table[(size_t)t * P + labels[index[i]]];
}

// The value-net step's batch: tf_out[i] as sl_batch, y_out[i] = values[index[i]] (the outcome
// is invariant under the board's symmetries).
__global__ void value_batch_kernel(const int64_t* __restrict__ index,
                                   const float* __restrict__ values,
                                   const int* __restrict__ sym, int nsym, uint32_t seed,
                                   uint32_t step, int* __restrict__ tf_out,
                                   float* __restrict__ y_out, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const uint32_t h = mix32(seed ^ mix32(step * 0x9E3779B9u + (uint32_t)i * 0x85EBCA6Bu + 1u));
  tf_out[i] = sym[h % (uint32_t)nsym];
  y_out[i] = values[index[i]];
}

// The SL step's batch with visit-count targets: one block per sampled row. tf_out[i] as
// sl_batch (same hash: a run can switch targets and keep its augmentation); the row's counts
// v [CD] (u16) become targets_out[i] [C] (fp32): v[p] / sum at the transformed point
// tf_table[t][p], the pass column (index P, when both have one) in place. A stored pass count
// that the model has no class for (CD = P + 1, C = P) is left out of the sum; a model pass class
// without a stored count (CD = P, C = P + 1) gets 0. A zero-sum row gives an all-zero row.
constexpr int kSoftBatchThreads = 256;

__global__ void __launch_bounds__(kSoftBatchThreads)
sl_batch_soft_kernel(const int64_t* __restrict__ index, const uint16_t* __restrict__ visits,
                     int CD, const int64_t* __restrict__ tf_table, int P,
                     const int* __restrict__ sym, int nsym, uint32_t seed, uint32_t step,
                     int* __restrict__ tf_out, float* __restrict__ targets_out, int C) {
  __shared__ uint32_t red[kSoftBatchThreads / 64];
  const int i = blockIdx.x;
  const uint32_t h = mix32(seed ^ mix32(step * 0x9E3779B9u + (uint32_t)i * 0x85EBCA6Bu + 1u));
  const int t = sym[h % (uint32_t)nsym];
  if (threadIdx.x == 0) tf_out[i] = t;
  const uint16_t* row = visits + (size_t)index[i] * CD;
  const int n = CD < C ? CD : C;  // the columns that count
  uint32_t s = 0;                 // <= 626 * 65535: exact
  for (int p = threadIdx.x; p < n; p += kSoftBatchThreads) s += row[p];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  uint32_t total = 0;
  for (int k = 0; k < kSoftBatchThreads / 64; ++k) total += red[k];
  const float den = (float)total;
  float* out = targets_out + (size_t)i * C;
  for (int p = threadIdx.x; p < C; p += kSoftBatchThreads) {
    const float v = (p < n && total) ? (float)row[p] / den : 0.f;
    out[p < P ? (int)tf_table[(size_t)t * P + p] : p] = v;
  }
}

}  // namespace

RAG_API int rag_sl_batch_soft(const int64_t* index, const uint16_t* visits, int CD,
                              const int64_t* tf_table, int P, const int* sym, int nsym,
                              unsigned seed, unsigned step, int* tf_out, float* targets_out,
                              int C, int B, hipStream_t stream) {
  if (nsym <= 0 || P <= 0) return -1;
  if ((CD != P && CD != P + 1) || (C != P && C != P + 1)) return -1;
  if (B <= 0) return 0;
  sl_batch_soft_kernel<<<B, kSoftBatchThreads, 0, stream>>>(index, visits, CD, tf_table, P, sym,
                                                            nsym, seed, step, tf_out,
                                                            targets_out, C);
  return (int)hipGetLastError();
}

RAG_API int rag_value_batch(const int64_t* index, const float* values, const int* sym, int nsym,
                            unsigned seed, unsigned step, int* tf_out, float* y_out, int B,
                            hipStream_t stream) {
  if (B <= 0) return 0;
  if (nsym <= 0) return -1;
  value_batch_kernel<<<(B + 255) / 256, 256, 0, stream>>>(index, values, sym, nsym, seed, step,
                                                          tf_out, y_out, B);
  return (int)hipGetLastError();
}

RAG_API int rag_sl_batch(const int64_t* index, const int64_t* labels, const int64_t* tf_table,
                         int P, const int* sym, int nsym, unsigned seed, unsigned step,
                         int* tf_out, int64_t* lab_out, int B, hipStream_t stream) {
  if (B <= 0) return 0;
  if (nsym <= 0 || P <= 0) return -1;
  sl_batch_kernel<<<(B + 255) / 256, 256, 0, stream>>>(index, labels, tf_table, P, sym, nsym,
                                                       seed, step, tf_out, lab_out, B);
  return (int)hipGetLastError();
}
