// Training of the Dense(relu) ... Dense(softmax) classifier on device: the step behind
// train_model (the reference's src/experiments/*/model.py: Keras Adam on the mean
// cross-entropy).  One optimiser step is two launches:
//
//   k_train<true>  (k_train_grad)  forward, backward and the weight gradient of one batch.  A
//       wave owns 16-row tiles as in k_pgd; a workgroup of wpb waves takes a contiguous run
//       of wpb * tpw tiles and works on wpb of them at a time (a round).  Per round every wave
//       leaves its tile's activations A_l and dZ_l in LDS; then the workgroup's waves share
//       out the 16 x 16 blocks of dW_l = A_l^T . dZ_l: a block's owner sums the round's tiles
//       in slot order on v_mfma_f32_16x16x4f32 (the contraction runs over a tile's 16 rows:
//       four issues per tile) and adds the sum to the workgroup's row of the partial scratch,
//       which the same lane wrote in the round before.  The last (softmax) layer's <= 8
//       columns, the biases and the loss run on the VALU, in the same fixed order.
//   k_train_adam   one thread per parameter: the workgroup partials summed in workgroup
//       order, then Keras-form Adam; thread 0 reduces the loss partials the same way.
//
// No atomics, no grid barrier: the reduced gradient depends on the batch and the plan alone.
// k_train<false> (k_train_eval) is the forward pass with the per-workgroup loss and
// argmax-correct count.
//
// The forward and backward tile functions restate pgd.hip's (kept apart so that file's
// bit-exact tests cannot move); fp32 throughout, built with -ffp-contract=off.  Rows past the
// end of the batch are loaded as zeros with d loss / d logit = 0: every product they enter is
// an exact zero.
#include <hip/hip_runtime.h>

#include "train.h"
#include "wave.h"

namespace mv {

typedef float trn_f4 __attribute__((ext_vector_type(4)));

namespace {

// One tile's LDS slice (pointers into the dynamic LDS block).
struct TrainTile {
  float* xs;                      // [16][Dp] scaled rows (A_0)
  float* h[PGD_MAX_LAYERS];       // h[l]: [16][dims[l] + 1] post-ReLU activations A_l, l >= 1
  float* dz[PGD_MAX_LAYERS];      // dz[l]: [16][dims[l + 1] + 1] d loss / d Z_l, l <= L - 2
  float* dl;                      // [16][PGD_MAX_OUT] d loss / d logit (dZ_{L-1})
  float* lossc;                   // [16] cross-entropy (0 on a dead row)
  int* ys;                        // [16] labels, then [16] argmax-correct flags
};

struct TrainLds {
  const float* W[PGD_MAX_LAYERS];  // LDS (staged) or global
  int ldw[PGD_MAX_LAYERS];
  float* tiles;
  size_t per;
};

__host__ __device__ inline size_t train_tile_floats(const TrainArgs& a) {
  size_t per = (size_t)PGD_ROWS * a.Dp + PGD_ROWS * PGD_MAX_OUT + 3 * PGD_ROWS;
  for (int l = 1; l < a.n_layers; ++l) per += (size_t)2 * PGD_ROWS * (a.dims[l] + 1);
  return per;
}

__device__ __forceinline__ void train_tile(const TrainArgs& a, const TrainLds& s, int slot,
                                           TrainTile& t) {
  float* p = s.tiles + s.per * slot;
  t.xs = p; p += PGD_ROWS * a.Dp;
  for (int l = 1; l < a.n_layers; ++l) {
    t.h[l] = p;
    p += PGD_ROWS * (a.dims[l] + 1);
  }
  for (int l = 0; l < a.n_layers - 1; ++l) {
    t.dz[l] = p;
    p += PGD_ROWS * (a.dims[l + 1] + 1);
  }
  t.dl = p; p += PGD_ROWS * PGD_MAX_OUT;
  t.lossc = p; p += PGD_ROWS;
  t.ys = (int*)p;
}

// Weights into LDS (row stride N + 1: the forward read W[k][col] and the transposed backward
// read W[col][k] are both conflict free); a first layer too large is streamed from L2.
__device__ __forceinline__ void train_setup(const TrainArgs& a, float* smem, TrainLds& s) {
  float* p = smem;
  for (int l = 0; l < a.n_layers; ++l) {
    const int K = a.dims[l], N = a.dims[l + 1];
    const float* Wg = a.params + a.off_w[l];
    if (l == 0 && !a.stage_w0) {
      s.W[l] = Wg;
      s.ldw[l] = N;
      continue;
    }
    const int ld = N + 1;
    for (int i = threadIdx.x; i < K * N; i += blockDim.x) p[(i / N) * ld + i % N] = Wg[i];
    s.W[l] = p;
    s.ldw[l] = ld;
    p += K * ld;
  }
  s.tiles = p;
  s.per = train_tile_floats(a);
  __syncthreads();
}

// out[16][N] = relu(in[16][K] . W[K][N] + bias), N % 16 == 0.  A operand lane (il, ka) holds
// in[il][k0 + ka], B operand W[k0 + ka][col tile + il]; acc[j] is row ka * 4 + j, column il.
__device__ __forceinline__ void dense_fwd(const float* in, int ldi, int K, const float* W,
                                          int ldw, const float* __restrict__ bias, int N,
                                          float* out, int ldo, int lane) {
  const int ka = lane >> 4, il = lane & 15;
  const int nct = N >> 4;
  for (int c0 = 0; c0 < nct; c0 += 4) {
    trn_f4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = trn_f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
      const int k = k0 + ka;
      const bool ok = k < K;
      const float av = ok ? in[il * ldi + k] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c0 + c < nct) {
          const float bv = ok ? W[(size_t)k * ldw + (c0 + c) * 16 + il] : 0.f;
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[c], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c0 + c < nct) {
        const int col = (c0 + c) * 16 + il;
        const float bv = bias[col];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = acc[c][j] + bv;
          out[(ka * 4 + j) * ldo + col] = v > 0.f ? v : 0.f;
        }
      }
    }
  }
}

// din[16][K] = dz[16][N] . W^T (W [K][N]), N % 16 == 0, K % 16 == 0, masked by hprev > 0
// (relu'(0) = 0).  B operand lane (il, ka) holds W[col tile + il][n0 + ka].
__device__ __forceinline__ void dense_bwd(const float* dz, int ldz, int N, const float* W,
                                          int ldw, int K, const float* hprev, int ldh,
                                          float* din, int ldd, int lane) {
  const int ka = lane >> 4, il = lane & 15;
  const int nct = K >> 4;
  for (int c0 = 0; c0 < nct; c0 += 4) {
    trn_f4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = trn_f4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < N; n0 += 4) {
      const float av = dz[il * ldz + n0 + ka];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c0 + c < nct) {
          const float bv = W[(size_t)((c0 + c) * 16 + il) * ldw + n0 + ka];
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[c], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c0 + c < nct) {
        const int col = (c0 + c) * 16 + il;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = ka * 4 + j;
          din[row * ldd + col] = hprev[row * ldh + col] > 0.f ? acc[c][j] : 0.f;
        }
      }
    }
  }
}

// Batch rows row0 .. row0 + 15 into t.xs (rows past the batch: zeros), labels into t.ys.
// A source row index is clamped into x, so a bad perm entry cannot leave the buffers.
__device__ __forceinline__ void train_load(const TrainArgs& a, const TrainTile& t, int lane,
                                           int row0) {
  for (int r = 0; r < PGD_ROWS; ++r) {
    const bool live = row0 + r < a.n;
    int src = 0;
    if (live) {
      src = a.perm ? a.perm[a.first + row0 + r] : a.first + row0 + r;
      src = src < 0 ? 0 : (src >= a.n_total ? a.n_total - 1 : src);
    }
    for (int f = lane; f < a.D; f += 64)
      t.xs[r * a.Dp + f] = live ? a.x[(size_t)src * a.D + f] : 0.f;
    if (lane == 0) {
      int y = 0;
      if (live) {
        y = a.y[src];
        const int no = a.dims[a.n_layers];
        y = y < 0 ? 0 : (y >= no ? no - 1 : y);
      }
      t.ys[r] = y;
    }
  }
  wave_sync();
}

// Hidden layers forward: t.xs -> t.h[1 .. L-1].
__device__ __forceinline__ void train_forward(const TrainArgs& a, const TrainLds& s,
                                              const TrainTile& t, int lane) {
  const int L = a.n_layers;
  for (int l = 0; l < L - 1; ++l) {
    const float* in = l == 0 ? t.xs : t.h[l];
    const int ldi = l == 0 ? a.Dp : a.dims[l] + 1;
    dense_fwd(in, ldi, a.dims[l], s.W[l], s.ldw[l], a.params + a.off_b[l], a.dims[l + 1],
              t.h[l + 1], a.dims[l + 1] + 1, lane);
    wave_sync();
  }
}

// Last layer on lanes 0..15 (one row each): logits, the cross-entropy from the logits, the
// argmax-correct flag (first maximum) and d mean-loss / d logit = (softmax - onehot) / rows.
// A row past the batch gets loss 0, flag 0 and a zero gradient.
__device__ __forceinline__ void train_last(const TrainArgs& a, const TrainLds& s,
                                           const TrainTile& t, int lane, int row0) {
  const int L = a.n_layers;
  const int K = a.dims[L - 1], no = a.dims[L];
  if (lane < PGD_ROWS) {
    const bool live = row0 + lane < a.n;
    const float* hr = t.h[L - 1] + lane * (K + 1);
    const float* W = s.W[L - 1];
    const int ldw = s.ldw[L - 1];
    const float* bias = a.params + a.off_b[L - 1];
    float z[PGD_MAX_OUT];
    float mx = -__builtin_inff();
    int am = 0;
#pragma unroll
    for (int c = 0; c < PGD_MAX_OUT; ++c) {
      z[c] = 0.f;
      if (c < no) {
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum = fmaf(hr[k], W[k * ldw + c], sum);
        z[c] = sum + bias[c];
        if (z[c] > mx) {
          mx = z[c];
          am = c;
        }
      }
    }
    const int y = t.ys[lane];
    float e[PGD_MAX_OUT];
    float S = 0.f, zy = 0.f;
#pragma unroll
    for (int c = 0; c < PGD_MAX_OUT; ++c) {
      e[c] = 0.f;
      if (c < no) {
        e[c] = expf(z[c] - mx);
        S = S + e[c];
        if (c == y) zy = z[c];
      }
    }
    t.lossc[lane] = live ? -((zy - mx) - logf(S)) : 0.f;
    t.ys[PGD_ROWS + lane] = live && am == y ? 1 : 0;
    const float rows = (float)a.n;
#pragma unroll
    for (int c = 0; c < PGD_MAX_OUT; ++c)
      if (c < no)
        t.dl[lane * PGD_MAX_OUT + c] = live ? (e[c] / S - (c == y ? 1.f : 0.f)) / rows : 0.f;
  }
  wave_sync();
}

// Backward through the hidden layers: t.dl -> t.dz[L-2 .. 0].
__device__ __forceinline__ void train_backward(const TrainArgs& a, const TrainLds& s,
                                               const TrainTile& t, int lane) {
  const int L = a.n_layers;
  const int ka = lane >> 4, il = lane & 15;
  {  // last layer: dz[L-2][row][k] = sum_c dl[row][c] W[k][c], masked by h[L-1] > 0
    const int K = a.dims[L - 1], no = a.dims[L];
    const float* W = s.W[L - 1];
    const int ldw = s.ldw[L - 1];
    for (int k = ka; k < K; k += 4) {
      float sum = 0.f;
      for (int c = 0; c < no; ++c) sum = fmaf(t.dl[il * PGD_MAX_OUT + c], W[k * ldw + c], sum);
      t.dz[L - 2][il * (K + 1) + k] = t.h[L - 1][il * (K + 1) + k] > 0.f ? sum : 0.f;
    }
    wave_sync();
  }
  for (int l = L - 2; l >= 1; --l) {
    dense_bwd(t.dz[l], a.dims[l + 1] + 1, a.dims[l + 1], s.W[l], s.ldw[l], a.dims[l], t.h[l],
              a.dims[l] + 1, t.dz[l - 1], a.dims[l] + 1, lane);
    wave_sync();
  }
}

// The round's weight gradient, added to the workgroup's partial row `part`: nlive tile slots
// hold A_l and dZ_l.  Work items are dealt to the waves (MFMA blocks) or threads (VALU sums)
// by a rule that does not depend on the round, so a partial entry has one owner throughout.
__device__ __forceinline__ void train_wgrad(const TrainArgs& a, const TrainLds& s, int nlive,
                                            bool first, float* part) {
  const int L = a.n_layers;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int ka = lane >> 4, il = lane & 15;
  TrainTile t;
  for (int l = 0; l < L - 1; ++l) {
    const int K = a.dims[l], N = a.dims[l + 1];
    const int lda = l == 0 ? a.Dp : K + 1, ldz = N + 1;
    const int nI = (K + 15) >> 4, nJ = N >> 4;
    float* dW = part + a.off_w[l];
    // dW_l[i][j] = sum_rows A_l[row][i] dZ_l[row][j]: A operand lane (il, ka) holds
    // A_l[q * 4 + ka][I * 16 + il], B operand dZ_l[q * 4 + ka][J * 16 + il]
    for (int blk = wave; blk < nI * nJ; blk += nw) {
      const int I = blk / nJ, J = blk - I * nJ;
      const int i = I * 16 + il;
      const bool ok = i < K;
      trn_f4 acc = trn_f4{0.f, 0.f, 0.f, 0.f};
      for (int slot = 0; slot < nlive; ++slot) {
        train_tile(a, s, slot, t);
        const float* A = l == 0 ? t.xs : t.h[l];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = q * 4 + ka;
          const float av = ok ? A[r * lda + i] : 0.f;
          const float bv = t.dz[l][r * ldz + J * 16 + il];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = I * 16 + ka * 4 + j;
        if (row < K) {
          float* d = dW + (size_t)row * N + J * 16 + il;
          *d = first ? acc[j] : *d + acc[j];
        }
      }
    }
    // db_l[j] = sum_rows dZ_l[row][j]
    float* db = part + a.off_b[l];
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
      float sum = 0.f;
      for (int slot = 0; slot < nlive; ++slot) {
        train_tile(a, s, slot, t);
        for (int r = 0; r < PGD_ROWS; ++r) sum = sum + t.dz[l][r * ldz + j];
      }
      db[j] = first ? sum : db[j] + sum;
    }
  }
  {  // last layer: no <= 8 columns
    const int K = a.dims[L - 1], no = a.dims[L];
    float* dW = part + a.off_w[L - 1];
    for (int idx = threadIdx.x; idx < K * no; idx += blockDim.x) {
      const int k = idx / no, c = idx - k * no;
      float sum = 0.f;
      for (int slot = 0; slot < nlive; ++slot) {
        train_tile(a, s, slot, t);
        for (int r = 0; r < PGD_ROWS; ++r)
          sum = fmaf(t.h[L - 1][r * (K + 1) + k], t.dl[r * PGD_MAX_OUT + c], sum);
      }
      dW[idx] = first ? sum : dW[idx] + sum;
    }
    float* db = part + a.off_b[L - 1];
    for (int c = threadIdx.x; c < no; c += blockDim.x) {
      float sum = 0.f;
      for (int slot = 0; slot < nlive; ++slot) {
        train_tile(a, s, slot, t);
        for (int r = 0; r < PGD_ROWS; ++r) sum = sum + t.dl[r * PGD_MAX_OUT + c];
      }
      db[c] = first ? sum : db[c] + sum;
    }
  }
}

}  // namespace

template <bool TRAIN>
__global__ __launch_bounds__(64 * PGD_MAX_WAVES) void k_train(const TrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float train_smem[];
  TrainLds s;
  train_setup(a, train_smem, s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles = (a.n + PGD_ROWS - 1) / PGD_ROWS;
  float* part = TRAIN ? a.partial + (size_t)blockIdx.x * a.n_params : nullptr;
  float loss = 0.f, correct = 0.f;  // thread 0
  TrainTile t;
  for (int round = 0; round < a.tpw; ++round) {
    const int tile0 = (blockIdx.x * a.tpw + round) * a.wpb;
    int nlive = tiles - tile0;
    nlive = nlive > a.wpb ? a.wpb : nlive;
    if (nlive <= 0) break;  // uniform over the workgroup; round 0 always has a tile
    if (wave < nlive) {
      const int row0 = (tile0 + wave) * PGD_ROWS;
      train_tile(a, s, wave, t);
      train_load(a, t, lane, row0);
      train_forward(a, s, t, lane);
      train_last(a, s, t, lane, row0);
      if (TRAIN) train_backward(a, s, t, lane);
    }
    __syncthreads();
    if (TRAIN) train_wgrad(a, s, nlive, round == 0, part);
    if (threadIdx.x == 0) {
      for (int slot = 0; slot < nlive; ++slot) {
        train_tile(a, s, slot, t);
        for (int r = 0; r < PGD_ROWS; ++r) {
          loss = loss + t.lossc[r];
          correct = correct + (float)t.ys[PGD_ROWS + r];
        }
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.loss_partial[2 * blockIdx.x] = loss;
    a.loss_partial[2 * blockIdx.x + 1] = correct;
  }
}

// One thread per parameter: g = the partials summed in workgroup order; then the reduced
// gradient (grad_out) and / or Keras-form Adam (params).  Thread 0: the loss partials.
__global__ __launch_bounds__(256) void k_train_adam(const AdamArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    float loss = 0.f, correct = 0.f;
    for (int g = 0; g < a.groups; ++g) {
      loss = loss + a.loss_partial[2 * g];
      correct = correct + a.loss_partial[2 * g + 1];
    }
    if (a.loss_out) *a.loss_out = loss / a.rows;
    if (a.correct_out) *a.correct_out = correct;
  }
  if (i >= a.n_params || !a.partial) return;
  float g = 0.f;
  for (int k = 0; k < a.groups; ++k) g = g + a.partial[(size_t)k * a.n_params + i];
  if (a.grad_out) a.grad_out[i] = g;
  if (a.params) {
    const float m = a.beta1 * a.m[i] + (1.f - a.beta1) * g;
    const float v = a.beta2 * a.v[i] + (1.f - a.beta2) * (g * g);
    a.m[i] = m;
    a.v[i] = v;
    a.params[i] = a.params[i] - (a.lr_t * m) / (sqrtf(v) + a.epsilon);
  }
}

static size_t train_weight_floats(const TrainArgs& a) {
  size_t w = 0;
  for (int l = 0; l < a.n_layers; ++l)
    if (l > 0 || a.stage_w0) w += (size_t)a.dims[l] * (a.dims[l + 1] + 1);
  return w;
}

size_t train_lds_bytes(const TrainArgs& a) {
  return (train_weight_floats(a) + train_tile_floats(a) * (size_t)a.wpb) * sizeof(float);
}

hipError_t train_plan_model(TrainArgs& a) {
  a.wpb = 1;
  a.tpw = 1;
  a.stage_w0 = 1;
  if (train_lds_bytes(a) > (size_t)PGD_LDS_BYTES) a.stage_w0 = 0;
  if (train_lds_bytes(a) > (size_t)PGD_LDS_BYTES) return hipErrorInvalidValue;
  return hipSuccess;
}

// As many waves per workgroup as fit in LDS (the fewer workgroups, the fewer partial rows),
// then tiles per wave so that the batch takes at most TRAIN_MAX_GROUPS workgroups.
static void train_plan(TrainArgs& a) {
  const int tiles = (a.n + PGD_ROWS - 1) / PGD_ROWS;
  a.wpb = tiles < PGD_MAX_WAVES ? tiles : PGD_MAX_WAVES;
  while (a.wpb > 1 && train_lds_bytes(a) > (size_t)PGD_LDS_BYTES) --a.wpb;
  a.tpw = (tiles + a.wpb * TRAIN_MAX_GROUPS - 1) / (a.wpb * TRAIN_MAX_GROUPS);
  a.groups = (tiles + a.wpb * a.tpw - 1) / (a.wpb * a.tpw);
}

template <class Kern>
static hipError_t train_launch(Kern kern, TrainArgs& a, hipStream_t stream) {
  if (a.n <= 0) return hipErrorInvalidValue;
  train_plan(a);
  const size_t lds = train_lds_bytes(a);
  if (lds > (size_t)PGD_LDS_BYTES || a.groups > TRAIN_MAX_GROUPS) return hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(
        (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, PGD_LDS_BYTES);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(a.groups), dim3(64 * a.wpb), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_train_grad(TrainArgs& a, hipStream_t stream) {
  return train_launch(k_train<true>, a, stream);
}

hipError_t launch_train_eval(TrainArgs& a, hipStream_t stream) {
  return train_launch(k_train<false>, a, stream);
}

hipError_t launch_train_adam(const AdamArgs& a, hipStream_t stream) {
  const int n = a.partial ? a.n_params : 1;
  hipLaunchKernelGGL(k_train_adam, dim3((n + 255) / 256), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mv
