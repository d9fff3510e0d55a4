// sgk_learn.hip -- DeepQAgent.learn (reference value.py:113-136) for the reference's default topology as ONE kernel:
// sample a minibatch from the device replay ring, forward the Q-network and the target network, the TD target and the MSE
// loss, the backward pass, clip_grad_norm_(10) and the Adam(amsgrad) update -- what PyTorch runs as ~80 small kernels
// (a 64-sample minibatch through a 36-100-100-4 MLP: every kernel is launch latency). One workgroup of 1 024 lanes; the
// minibatch, both networks' activations and the two back-propagated activations live in LDS, every lane keeps the
// gradients of the parameters it owns in registers, and the weights are read from L2 in the orientation that makes the
// lanes' addresses consecutive (a transposed copy of W1 / W2 / W3 is kept current by the update itself; the fused policy
// kernels read W1^T and W3^T from it).
//
// fp32 throughout, same formulas as torch (mse_loss over the [B,1]-vs-[B] broadcast of value.py:119-123 by default -- loss_mode,
// see the kernel; clip coefficient max_norm / (norm + 1e-6) clamped to 1, Adam with bias corrections and amsgrad); the summation
// order inside the dot products differs from rocBLAS / torch's CPU kernels, so parity is to fp32 tolerance, not bit for bit: the
// reference's own DeepQAgent runs (tests/golden/batched_dqn_*.npz, 320-330 steps across three target syncs) are reproduced with
// every action equal, losses and weights within rtol 2e-4 (tests/test_gpu_batched_golden.py).
#include <algorithm>
#include <type_traits>

#include "sgk_device.h"
#include "sgk_step_store.h"

extern "C" __device__ float __ockl_wfred_add_f32(float);

namespace sgk {

// -DSGK_LEARN_TIMELINE (tools/gpu_dqn_timeline.sh builds it into a library of its own, never the product's): lane 0 stamps
// wall_clock64() (100 MHz) behind every barrier of dqn_sgd_kernel; sgk_debug_learn_stamps() reads them back.
#ifdef SGK_LEARN_TIMELINE
__device__ unsigned long long learn_stamps[32];
// (stamps 30 / 31: the shader clock counter, s_memtime, at the first and at the latest stamp: in-kernel clock = their difference over
// the wall-clock difference x 100 MHz)
#define SGK_STAMP(i) do { if (threadIdx.x == 0) { learn_stamps[i] = wall_clock64(); learn_stamps[(i) == 0 ? 30 : 31] = __builtin_amdgcn_s_memtime(); } } while (0)
#else
#define SGK_STAMP(i) do { } while (0)
#endif

constexpr int LWG = 1024;    // lanes of the one workgroup
constexpr int LB = 64;       // samples per minibatch handled (batch <= 64)

struct LearnArgs {
  // replay ring [slices][n_envs][...]
  const int8_t *states, *successors;
  const uint8_t *actions;
  const int8_t *rewards;
  const uint8_t *terminals;
  int64_t n_envs, total;  // sampling range: total = filled slices * n_envs
  int32_t n_cells;
  // Q-network (torch layouts [out][in]) updated in place; transposed copies kept current; Adam state per tensor
  float *w1, *b1, *w2, *b2, *w3, *b3;
  float *w1t, *w2t, *w3t;
  float *m[6], *v[6], *vmax[6];  // order: w1, b1, w2, b2, w3, b3
  // target network: transposed hidden weights, output weights as they are [4][H]
  const float *tw1t, *tb1, *tw2t, *tb2, *tw3, *tb3;
  long long *step;   // Adam step counter on the device
  float *loss_out;   // may be null
  const long long *rows;  // the caller's minibatch (transition indices into the ring), or null: drawn here
  long long *rows_out;    // the minibatch used, or null
  float *adam_scratch;    // null: Adam inside dqn_sgd_kernel; else AdamHeader + the flat gradient go here and dqn_adam_kernel follows
  int32_t n_hidden, batch;
  int32_t loss_mode;  // 0 = the reference's [B,1]-vs-[B] broadcast mse_loss (value.py:119-123), 1 = per-sample (squeezed) mse_loss
  uint64_t seed;  // minibatch indices: Philox stream 4, ctr = {sample, 0, Adam step before this update, 4}
  float lr, beta1, beta2, eps, discount, max_norm;
  double reward_scale;  // what one unit of the int8 rewards is worth (SgkRules.reward_scale; 1 except tomato watering): the
                        // reference's reward is the float64 product, rounded to float32 when the batch tensor is made (value.py:170-171)
  // sgk_dqn_sgd_step_members: one workgroup per member (see MemberOffsets); one member: member_envs = n_envs, member_total = total
  int64_t member_envs, member_total;  // E = n_envs / n_members; the draw's range, filled slices * E
  const uint64_t *member_keys;        // [n_members] Philox keys of the members' draws; null: `seed` for every member
  int64_t scratch_stride;             // floats between two members' slices of adam_scratch
  // sgk_dqn_sgd_step_members_hyper (the HYPER instantiation only): [n_members], member m's lr and discount instead of the two above
  const DqnMemberHyper *member_hyper;
};

typedef float f4 __attribute__((ext_vector_type(4)));

// Cooperative global -> LDS copy of n floats (n % 4 == 0, both 16-byte aligned): every lane's loads are in flight together,
// ONE memory round trip for the whole block. The kernel is a chain of dependent phases run by a single workgroup, so what
// it costs is (number of exposed round trips) x (latency): reading the weights straight from L2 inside the dot-product
// loops was 80 round trips = 85-180 us; staged like this the kernel has about ten.
__device__ __forceinline__ void stage(float *dst, const float *__restrict__ src, int n) {
  for (int i = threadIdx.x * 4; i < n; i += LWG * 4) *reinterpret_cast<f4 *>(dst + i) = *reinterpret_cast<const f4 *>(src + i);
}

// Row stride of a staged weight matrix [rows][H]: H padded so that stride % 32 == 8. The MFMA A operand of dense_layer is
// wt[(4 u + grp) * stride + n0 + col] over the lanes (col = 0..15, grp = 0..3): with stride 100 the four groups start 4 banks
// apart and overlap (up to 4 lanes per bank: four LDS passes), with stride % 32 == 8 they tile the 32 banks exactly (two
// lanes per bank, the minimum for 64 lanes).
constexpr int weight_stride(int h) { return h + (40 - h % 32) % 32; }

// stage() for a [rows][H] matrix into rows of weight_stride(H) floats
template <int H>
__device__ __forceinline__ void stage_rows(float *dst, const float *__restrict__ src, int rows) {
  constexpr int WS = weight_stride(H);
  for (int i = threadIdx.x * 4; i < rows * H; i += LWG * 4) {
    const int r = i / H, c = i - r * H;
    *reinterpret_cast<f4 *>(dst + r * WS + c) = *reinterpret_cast<const f4 *>(src + i);
  }
}

// stage_rows() in two halves: the loads into registers BEFORE a compute phase, the LDS stores behind it -- the matrix's trip from
// L2 runs in the shadow of the phase instead of in front of the next one (one staging buffer, re-filled per layer: the
// activations of 64 samples leave LDS no room for a second)
template <int H, int ROWS>
struct RowsInFlight {
  static constexpr int N = (ROWS * H / 4 + LWG - 1) / LWG;
  f4 v[N];
};
template <int H, int ROWS>
__device__ __forceinline__ void rows_request(RowsInFlight<H, ROWS> &r, const float *__restrict__ src) {
#pragma unroll
  for (int n = 0; n < RowsInFlight<H, ROWS>::N; ++n) {
    const int i = ((int)threadIdx.x + n * LWG) * 4;
    r.v[n] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    if (i < ROWS * H) r.v[n] = *reinterpret_cast<const f4 *>(src + i);
  }
}
template <int H, int ROWS>
__device__ __forceinline__ void rows_commit(float *dst, const RowsInFlight<H, ROWS> &r) {
  constexpr int WS = weight_stride(H);
#pragma unroll
  for (int n = 0; n < RowsInFlight<H, ROWS>::N; ++n) {
    const int i = ((int)threadIdx.x + n * LWG) * 4;
    if (i < ROWS * H) {
      const int rr = i / H, c = i - rr * H;
      *reinterpret_cast<f4 *>(dst + rr * WS + c) = r.v[n];
    }
  }
}

__device__ __forceinline__ f4 load_x4(const float *row, int k) { return *reinterpret_cast<const f4 *>(row + k); }
__device__ __forceinline__ f4 load_x4(const int8_t *row, int k) {  // four board cells -> four floats
  const uint32_t w = *reinterpret_cast<const uint32_t *>(row + k);
  return (f4){(float)(int8_t)(w & 0xff), (float)(int8_t)((w >> 8) & 0xff), (float)(int8_t)((w >> 16) & 0xff), (float)(int8_t)(w >> 24)};
}

__device__ __forceinline__ float load_x1(const float *row, int k) { return row[k]; }
__device__ __forceinline__ float load_x1(const int8_t *row, int k) { return (float)row[k]; }

// out[b][n] = epilogue(bias[n] + sum_k in[b][k] * wt[k][n]) for the LB samples and n < H, everything in LDS, on the matrix
// cores (v_mfma_f32_16x16x4_f32: exact fp32): out^T = W in^T in 16 x 16 tiles, A operand = 16 neurons x 4 k of wt (lanes
// along n: consecutive words), B operand = 4 k x 16 samples of `in`, C = 16 neurons x 16 samples. Two 4-byte LDS reads feed
// 1 024 FMAs; the VALU form before it (4 neurons x 2 samples per lane) moved 3 bytes of LDS per FMA and spent 8.6 us per
// 100 x 100 layer on LDS bandwidth alone. The ceil(H / 16) x 4 output tiles are dealt round-robin to the 16 waves.
// KP = row stride of `in` in elements; `mask` zeroes out[b][n] where mask[b][n] <= 0 (ReLU'); neuron rows >= H of the last
// tile are computed from whatever lies behind the row (still inside LDS) and dropped.
template <int K, int H, int WST = H, class T>
__device__ __forceinline__ void dense_layer(const T *in, int KP, const float *wt, const float *bias, float *out, bool relu,
                                            const float *mask) {  // WST = row stride of wt
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  constexpr int MT = (H + 15) / 16, KS = (K + 3) / 4;  // neuron tiles, k-steps
  constexpr int CH = KS < 8 ? KS : 8;                    // k-steps whose operands are fetched together
  // (two tiles per wave in flight -- two independent accumulator chains behind one batch of 32 LDS reads -- was slower:
  // 41.5 -> 44.5 us for the DeepQ step, 653 -> 727 us for 16 PPO epochs)
  for (int tile = wave; tile < MT * (LB / 16); tile += n_waves) {
    const int n0 = 16 * (tile % MT), b0 = 16 * (tile / MT);
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bias && n0 + 4 * grp < H) acc = *reinterpret_cast<const f4 *>(bias + n0 + 4 * grp);
    const T *xrow = in + (b0 + col) * KP;
    const float *wcol = wt + n0 + col;
    // compile-time shapes: the loop nest unrolls completely and the operand reads of a chunk are issued before its MFMAs
    // (with a runtime K the compiler waited out every LDS read in front of the MFMA using it: 15 k cycles per 100 x 100
    // layer against an issue bound of 6.4 k)
#pragma unroll
    for (int c0 = 0; c0 < KS; c0 += CH) {
      float av[CH], bv[CH];
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const int k = 4 * (c0 + u) + grp;
        if (4 * (c0 + u) + 3 < K) {  // whole k-step inside K: no guard
          av[u] = wcol[k * WST];
          bv[u] = load_x1(xrow, k);
        } else if (4 * (c0 + u) < K) {  // the ragged last k-step
          const int kc = k < K ? k : K - 1;
          av[u] = k < K ? wcol[kc * WST] : 0.0f;
          bv[u] = k < K ? load_x1(xrow, kc) : 0.0f;
        } else {
          av[u] = 0.0f;
          bv[u] = 0.0f;
        }
      }
#pragma unroll
      for (int u = 0; u < CH; ++u)
        if (4 * (c0 + u) < K) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
    const int n = n0 + 4 * grp;  // this lane's four neurons, sample b0 + col
    if (n < H) {
      if (relu) acc = __builtin_elementwise_max(acc, (f4){0.0f, 0.0f, 0.0f, 0.0f});
      if (mask) {
        const f4 m = *reinterpret_cast<const f4 *>(mask + (b0 + col) * H + n);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = m[c] > 0.0f ? acc[c] : 0.0f;
      }
      *reinterpret_cast<f4 *>(out + (b0 + col) * H + n) = acc;
    }
  }
}

// q[b][a] = b3[a] + sum_k h[b][k] * w3[a][k] (all LDS): one lane per (b, a)
__device__ __forceinline__ void head_forward(const float *h, int H, const float *w3, const float *b3, float *q) {
  if (threadIdx.x < LB * 4) {
    const int b = threadIdx.x >> 2, a = threadIdx.x & 3;
    float acc = b3[a];
    for (int k0 = 0; k0 < H; k0 += 4) {  // H % 4 == 0 (checked by the launcher)
      const f4 w = *reinterpret_cast<const f4 *>(w3 + a * H + k0);
      const f4 x = *reinterpret_cast<const f4 *>(h + b * H + k0);
      acc = fmaf(x[0], w[0], acc);
      acc = fmaf(x[1], w[1], acc);
      acc = fmaf(x[2], w[2], acc);
      acc = fmaf(x[3], w[3], acc);
    }
    q[b * 4 + a] = acc;
  }
}

// grad[r][c] = sum_b d[b][row0 + r] * x[b][col0 + c] for a 4 x 4 tile (the weight gradient of a dense layer): two LDS reads
// per sample for 16 FMAs
template <class T>
__device__ __forceinline__ void weight_grad_tile(const float *d, int DS, int row0, const T *x, int XS, int col0, f4 g[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) g[r] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
  for (int b = 0; b < LB; ++b) {
    const f4 dv = *reinterpret_cast<const f4 *>(d + b * DS + row0);
    const f4 xv = load_x4(x + b * XS, col0);
#pragma unroll
    for (int r = 0; r < 4; ++r) g[r] = __builtin_elementwise_fma((f4){dv[r], dv[r], dv[r], dv[r]}, xv, g[r]);
  }
}

// One 16 x 16 tile of a weight gradient on the matrix cores: G[r][c] = sum_b d[b][row0 + r] * x[b][col0 + c] over the LB samples
// (K = the batch). A operand = d[b][row0 + (lane & 15)], B operand = x[b][col0 + (lane & 15)], b = 4 s + (lane >> 4): both
// are consecutive words across the lanes. Result in the C layout: lane (col, grp), register r = G[4 grp + r][col].
template <class T>
__device__ __forceinline__ f4 weight_grad_mfma(const float *d, int DS, int row0, const T *x, int XS, int col0, int lane) {
  const int col = lane & 15, grp = lane >> 4;
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  float av[LB / 4], bv[LB / 4];
#pragma unroll
  for (int s = 0; s < LB / 4; ++s) {
    av[s] = d[(4 * s + grp) * DS + row0 + col];
    bv[s] = load_x1(x + (4 * s + grp) * XS, col0 + col);
  }
#pragma unroll
  for (int s = 0; s < LB / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
  return acc;
}

// The same tile with the operands exchanged: the result comes out TRANSPOSED in the C layout -- lane (col, grp), register r =
// G[row0 + col][col0 + 4 grp + r]: four CONSECUTIVE columns of one row, i.e. 16 contiguous bytes of a row-major [rows][cols] tensor.
// The owner's Adam traffic on w, m, v and vmax is then four 16-byte loads and four 16-byte stores per quad instead of sixteen and
// sixteen dword ones (one CU's memory pipeline was what bounded that phase: 13 us for 13.9 k parameters).
template <class T>
__device__ __forceinline__ f4 weight_grad_mfma_t(const float *d, int DS, int row0, const T *x, int XS, int col0, int lane) {
  const int col = lane & 15, grp = lane >> 4;
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  float av[LB / 4], bv[LB / 4];
#pragma unroll
  for (int s = 0; s < LB / 4; ++s) {
    av[s] = load_x1(x + (4 * s + grp) * XS, col0 + col);
    bv[s] = d[(4 * s + grp) * DS + row0 + col];
  }
#pragma unroll
  for (int s = 0; s < LB / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
  return acc;
}

// Column sums on the matrix cores (a bias gradient): S[r] = sum_b d[b][row0 + r] over the LB samples -- the same tile product
// with a B operand of ones. Lane (col, grp), register r = S[4 grp + r], the same in every column. A 64-iteration serial loop
// per bias lane (64 dependent LDS reads, two waves busy, fourteen idle) cost 2-3 us per layer.
__device__ __forceinline__ f4 column_sum_mfma(const float *d, int DS, int row0, int lane) {
  const int col = lane & 15, grp = lane >> 4;
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  float av[LB / 4];
#pragma unroll
  for (int s = 0; s < LB / 4; ++s) av[s] = d[(4 * s + grp) * DS + row0 + col];
#pragma unroll
  for (int s = 0; s < LB / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], 1.0f, acc, 0, 0, 0);
  return acc;
}

__device__ __forceinline__ float block_sum(float x, float *scratch) {  // scratch: LWG / 64 floats
  x = __ockl_wfred_add_f32(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = x;
  __syncthreads();
  float total = 0.0f;
  for (int w = 0; w < LWG / 64; ++w) total += scratch[w];
  return total;
}

struct AdamCoef {
  float lr_bc1, inv_bc2_sqrt, beta1, beta2, eps;  // lr / bias_correction1, 1 / sqrt(bias_correction2)
};

// One element of Adam(amsgrad), torch's formulas: exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) grad^2;
// denom = sqrt(max_exp_avg_sq) / sqrt(bias_correction2) + eps; param -= lr / bias_correction1 * exp_avg / denom.
// The square root and the two quotients use the hardware's one-ulp forms (v_sqrt_f32, v_rcp_f32; 1 / sqrt(bias_correction2) is
// formed once per launch): with IEEE sqrtf() and `/` the phase was VALU-bound -- ~60 instructions per element, 28 element slots per
// lane, four waves per SIMD at four cycles per wave64 instruction = 11 of the 13 us the timeline showed -- and a relative 1e-7 in
// an update that is itself ~1e-3 of the weight is far inside what the float32 summation order already differs by.
__device__ __forceinline__ float adam_scalar(float p, float &m, float &v, float &vmax, float g, const AdamCoef &c) {
  m = m + (1.0f - c.beta1) * (g - m);
  v = c.beta2 * v + (1.0f - c.beta2) * g * g;
  vmax = fmaxf(vmax, v);
  const float denom = __builtin_amdgcn_sqrtf(vmax) * c.inv_bc2_sqrt + c.eps;
  return p - c.lr_bc1 * (m * __builtin_amdgcn_rcpf(denom));
}

// Adam on four consecutive parameters (16-byte aligned); returns the updated values
__device__ __forceinline__ f4 adam_row(float *p, float *m, float *v, float *vmax, f4 g, const AdamCoef &c) {
  f4 pv = *reinterpret_cast<f4 *>(p), mv = *reinterpret_cast<f4 *>(m), vv = *reinterpret_cast<f4 *>(v), xv = *reinterpret_cast<f4 *>(vmax);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float mi = mv[i], vi = vv[i], xi = xv[i];
    pv[i] = adam_scalar(pv[i], mi, vi, xi, g[i], c);
    mv[i] = mi; vv[i] = vi; xv[i] = xi;
  }
  *reinterpret_cast<f4 *>(p) = pv;
  *reinterpret_cast<f4 *>(m) = mv;
  *reinterpret_cast<f4 *>(v) = vv;
  *reinterpret_cast<f4 *>(vmax) = xv;
  return pv;
}

// LDS plan (floats unless noted): A, Bq, C, D [LB][H] -- A = Q hidden 1, Bq = Q hidden 2, C = target hidden 1 then dL/dh2,
// D = target hidden 2 then dL/dh1; ST [H][H] the weight matrix of the running phase; SM the small tensors (W3, target W3, the
// biases); S, S2 int8 [LB][KP] the boards; the per-sample scalars.
struct LearnLds {
  float *A, *Bq, *C, *D, *ST, *w3, *tw3, *b1, *b2, *b3, *tb1, *tb2, *tb3, *q, *tq, *y, *scratch, *rew;
  int8_t *S, *S2;
  int *idx, *act, *term;
};

__device__ __forceinline__ LearnLds carve(unsigned char *base, int KP, int H) {
  LearnLds L;
  float *f = reinterpret_cast<float *>(base);
  L.A = f; f += LB * H;
  L.Bq = f; f += LB * H;
  L.C = f; f += LB * H;
  L.D = f; f += LB * H;
  L.ST = f; f += H * weight_stride(H);
  L.w3 = f; f += 4 * H;
  L.tw3 = f; f += 4 * H;
  L.b1 = f; f += H;
  L.b2 = f; f += H;
  L.tb1 = f; f += H;
  L.tb2 = f; f += H;
  L.b3 = f; f += 4;
  L.tb3 = f; f += 4;
  L.q = f; f += LB * 4;
  L.tq = f; f += LB * 4;
  L.y = f; f += LB;
  L.scratch = f; f += 32;
  L.rew = f; f += LB;
  L.idx = reinterpret_cast<int *>(f); f += LB;
  L.act = reinterpret_cast<int *>(f); f += LB;
  L.term = reinterpret_cast<int *>(f); f += LB;
  L.S = reinterpret_cast<int8_t *>(f);
  L.S2 = L.S + LB * KP;
  return L;
}

// flat parameter vector in torch's registration order: w1 [H][K0], b1 [H], w2 [H][H], b2 [H], w3 [4][H], b3 [4]
template <int K0, int H>
struct ParamMap {
  static constexpr int o_w1 = 0, o_b1 = H * K0, o_w2 = o_b1 + H, o_b2 = o_w2 + H * H, o_w3 = o_b2 + H, o_b3 = o_w3 + 4 * H, P = o_b3 + 4;
};

// The member axis (sgk_dqn_sgd_step_members; one member = sgk_dqn_sgd_step, offsets of zero): every tensor of LearnArgs but the replay
// ring is stacked [n_members][...] and the pointers address member 0; a workgroup adds its member's offsets (wave-uniform address
// arithmetic). The ring is shared: member m owns the env columns m * E ..
// (m + 1) * E - 1 and draws from them alone. A workgroup of dqn_sgd_kernel fills a CU's LDS, so the members run one per CU and in
// waves above that; dqn_adam_kernel's grid is n_members x ceil(P / 256), workgroup -> (member, block).
template <int K0, int H>
struct MemberOffsets {  // in elements, by tensor shape: W1 / W1^T, a hidden bias, W2 / W2^T, W3 / W3^T, b3 (32-bit: launch_dqn_sgd checks)
  uint32_t mb;
  __device__ __forceinline__ uint32_t w1() const { return mb * (uint32_t)(H * K0); }
  __device__ __forceinline__ uint32_t b() const { return mb * (uint32_t)H; }
  __device__ __forceinline__ uint32_t w2() const { return mb * (uint32_t)(H * H); }
  __device__ __forceinline__ uint32_t w3() const { return mb * (uint32_t)(4 * H); }
  __device__ __forceinline__ uint32_t b3() const { return mb * 4u; }
  __device__ __forceinline__ uint32_t tensor(int ten) const { return ten == 0 ? w1() : ten == 2 ? w2() : ten == 4 ? w3() : ten == 5 ? b3() : b(); }
};

// Two launches instead of one (round 6): the SGD step's last phase -- Adam on 13.9 k parameters -- moves ~500 KB through ONE CU's
// vector-memory path and took 10 of the kernel's 39 us (profiles/r06/dqn_timeline.log). With a.adam_scratch set, dqn_sgd_kernel stops
// behind the norm: it stores the gradient (flat, torch's parameter order, 16 bytes per lane where the MFMA layout gives four
// consecutive elements) and {clip coefficient, lr / bias_correction1, 1 / sqrt(bias_correction2)} to the handle's scratch block, and
// dqn_adam_kernel -- one lane per parameter, every CU, coalesced -- applies the update behind the kernel boundary (a boundary costs
// ~1.5 us; a grid barrier inside one launch 6-8: EXPERIMENTS R6.4).
struct AdamHeader {
  float coef, lr_bc1, inv_bc2_sqrt, pad;
};

// MEMBERS = false is the launch of one workgroup (sgk_dqn_sgd_step, and sgk_dqn_sgd_step_members with one member): the member index is
// the constant 0 and every offset below folds away; MEMBERS = true is the same code with workgroup m serving member m.
// HYPER = true (sgk_dqn_sgd_step_members_hyper; with MEMBERS only) is MEMBERS = true with a.lr and a.discount replaced by member m's
// element of a.member_hyper, converted with the host's (float) cast: one 16-byte load at entry, requested in front of the gather and
// consumed behind it by the lane that forms the bias corrections -- every lane requests the same 16 bytes into VECTOR registers (the
// index is laundered): the kernel sits at the SGPR limit, and the same load into scalar registers made the compiler reload kernel
// arguments in front of the gather's requests (+1.0 us per call from a kernel trace), while requested where it is used it was one more
// exposed round trip (+0.3 .. 0.8 us). As it stands the instantiation costs +0.6 .. 0.75 us against MEMBERS alone (29.8 against 29.1 us
// at 16 members: profiles/member_hyper/new_vs_old.log). The discount is parked in LDS until the loss reads it: no register lives
// across the forward passes for it.
template <int K0, int H, bool MEMBERS = false, bool HYPER = false>
__global__ __launch_bounds__(LWG) void dqn_sgd_kernel(LearnArgs a) {
  static_assert(MEMBERS || !HYPER, "per-member hyper-parameters come with the member axis");
  SGK_STAMP(0);
  extern __shared__ __attribute__((aligned(16))) unsigned char learn_smem[];
  const int B = a.batch;
  constexpr int KP = (K0 + 3) & ~3;  // row stride of the board matrices (padding columns hold zeros)
  const LearnLds L = carve(learn_smem, KP, H);
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6, col = lane & 15, grp = lane >> 4;
  constexpr int MT = (H + 15) / 16, KT1 = (K0 + 15) / 16;  // 16-wide tiles along neurons / along board cells
  // this member's slice of every stacked tensor: `a` stays as it came (kernel arguments, read where they are used) and the member's
  // offsets are added at the uses (wave-uniform address arithmetic; a shifted copy of all 45 pointers would have to live in SGPRs)
  const size_t mb = MEMBERS ? blockIdx.x : 0;
  const MemberOffsets<K0, H> mo{(uint32_t)mb};
  const long long env0 = MEMBERS ? (long long)mb * a.member_envs : 0;  // this member's first env column
  const uint64_t seed = (MEMBERS && a.member_keys) ? a.member_keys[mb] : a.seed;
  using TransitionId = typename std::conditional<MEMBERS, long long, int>::type;  // (one member: below 2^31, sgk_dqn_sgd_step checks)

  // ---- entry: ONE dependent chain of two memory round trips (the Adam step counter, then everything keyed by it) ----
  // minibatch: uniform with replacement over the stored transitions (contain.py:19-22), counter RNG. The index of the sample whose
  // bytes a lane fetches is derived by that lane (16 lanes per sample, each the same draw): the board gather needs no exchange
  // through LDS behind the draw, so indices, scalars and both boards travel together (they were two round trips and a barrier).
  const long long step0 = a.step[mb];
  DqnMemberHyper hp{};
  if constexpr (HYPER) {
    int same = 0;
    asm volatile("" : "+v"(same));  // (a vector load: see above)
    hp = a.member_hyper[mb + same];
  }
  // the first weight matrix and the small tensors are independent of it: requested first, so that they are in flight meanwhile
  RowsInFlight<H, K0> first;
  rows_request<H, K0>(first, a.tw1t + mo.w1());
  stage(L.w3, a.w3 + mo.w3(), 4 * H);
  stage(L.tw3, a.tw3 + mo.w3(), 4 * H);
  stage(L.b1, a.b1 + mo.b(), H);
  stage(L.b2, a.b2 + mo.b(), H);
  stage(L.tb1, a.tb1 + mo.b(), H);
  stage(L.tb2, a.tb2 + mo.b(), H);
  if (t < 4) { L.b3[t] = a.b3[mo.b3() + t]; L.tb3[t] = a.tb3[mo.b3() + t]; }
  {
    const int b = t >> 4, kk = t & 15;  // sample, byte lane (64 samples x 16 lanes = the workgroup)
    // transitions are named by their GLOBAL index slice * n_envs + env; a member's draw `d` over its own filled slices * E transitions
    // names (d / E) * n_envs + env0 + d % E (one member: E = n_envs, env0 = 0: d itself)
    TransitionId id = (TransitionId)env0;
    if (b < B) {
      if (a.rows) {
        // (an index outside the stored transitions, or of an env that is not the member's own, reads the member's first transition --
        // slice 0, env env0: transition 0 with one member --, not wild memory)
        const long long r = a.rows[mb * (size_t)a.batch + b];
        if (r >= 0 && r < a.total) {
          const long long e = MEMBERS ? r % a.n_envs - env0 : 0;
          if (!MEMBERS || (e >= 0 && e < a.member_envs)) id = (TransitionId)r;
        }
      } else {
        uint32_t x[4];
        philox4x32_10((uint32_t)b, 0u, (uint32_t)step0, 4u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
        const unsigned long long r = ((unsigned long long)x[0] << 32) | x[1];
        const uint32_t d = (uint32_t)__umul64hi(r, (unsigned long long)(MEMBERS ? a.member_total : a.total));
        if constexpr (MEMBERS) {
          const uint32_t E = (uint32_t)a.member_envs, sl = d / E;
          id = (long long)sl * a.n_envs + env0 + (d - sl * E);
        } else id = (int)d;
      }
    }
    if (kk == 0) {
      if (b < B && a.rows_out) a.rows_out[mb * (size_t)a.batch + b] = id;
      L.act[b] = a.actions[id] & 3;
      L.rew[b] = (float)((double)a.rewards[id] * a.reward_scale);
      L.term[b] = a.terminals[id] ? 1 : 0;
    }
    int8_t sv[(KP + 15) / 16], s2v[(KP + 15) / 16];
#pragma unroll
    for (int j = 0; j < (KP + 15) / 16; ++j) {  // all of a lane's bytes requested before the first is used
      const int k = kk + 16 * j;
      const bool live = b < B && k < K0;
      sv[j] = live ? a.states[(int64_t)id * K0 + k] : (int8_t)0;
      s2v[j] = live ? a.successors[(int64_t)id * K0 + k] : (int8_t)0;
    }
#pragma unroll
    for (int j = 0; j < (KP + 15) / 16; ++j) {
      const int k = kk + 16 * j;
      if (k < KP) {
        L.S[b * KP + k] = sv[j];
        L.S2[b * KP + k] = s2v[j];
      }
    }
  }
  rows_commit<H, K0>(L.ST, first);
  if (t == LWG - 1) {  // Adam's bias corrections (two double-precision pow(), ~1.3 us on one lane) in the shadow of the gather
    const long long step = step0 + 1;
    float lr = a.lr;
    if constexpr (HYPER) {
      lr = (float)hp.lr;
      L.scratch[18] = (float)hp.discount;  // (block_sum uses scratch[0 .. 15], the bias corrections 16 and 17)
    }
    L.scratch[16] = lr / (float)(1.0 - pow((double)a.beta1, (double)step));
    L.scratch[17] = 1.0f / sqrtf((float)(1.0 - pow((double)a.beta2, (double)step)));
  }
  __syncthreads();
  SGK_STAMP(1);
  // ---- target network on the successors; every next matrix is requested before the layer that precedes its use ----
  RowsInFlight<H, H> big;
  RowsInFlight<H, K0> small;
  rows_request<H, H>(big, a.tw2t + mo.w2());
  dense_layer<K0, H, weight_stride(H)>(L.S2, KP, L.ST, L.tb1, L.C, true, nullptr);
  __syncthreads();
  SGK_STAMP(2);
  rows_commit<H, H>(L.ST, big);
  __syncthreads();
  SGK_STAMP(3);
  rows_request<H, K0>(small, a.w1t + mo.w1());
  dense_layer<H, H, weight_stride(H)>(L.C, H, L.ST, L.tb2, L.D, true, nullptr);
  __syncthreads();
  SGK_STAMP(4);
  head_forward(L.D, H, L.tw3, L.tb3, L.tq);
  // ---- Q-network on the states ----
  rows_commit<H, K0>(L.ST, small);
  __syncthreads();
  SGK_STAMP(5);
  rows_request<H, H>(big, a.w2t + mo.w2());
  dense_layer<K0, H, weight_stride(H)>(L.S, KP, L.ST, L.b1, L.A, true, nullptr);
  __syncthreads();
  SGK_STAMP(6);
  rows_commit<H, H>(L.ST, big);
  __syncthreads();
  SGK_STAMP(7);
  rows_request<H, H>(big, a.w2 + mo.w2());  // W2 as it is ([j][k]): the back-propagation through layer 2 wants it in this orientation
  dense_layer<H, H, weight_stride(H)>(L.A, H, L.ST, L.b2, L.Bq, true, nullptr);
  __syncthreads();
  SGK_STAMP(8);
  head_forward(L.Bq, H, L.w3, L.b3, L.q);
  rows_commit<H, H>(L.ST, big);
  __syncthreads();
  SGK_STAMP(9);
  // ---- the loss on y_j = r_j + discount * max_a' Q_target(s'_j, a') * (1 - terminal_j) and q_i = Q(s_i, a_i); dL/dq on the taken action.
  // loss_mode 0 (the reference, value.py:119-123): Qs is [B,1] and expected_Qs [B], so F.mse_loss broadcasts them to [B,B]:
  //   loss = mean_{i,j} (q_i - y_j)^2 = mean_i (q_i - ybar)^2 + mean_j (y_j - ybar)^2,   dL/dq_i = (2 / B) (q_i - ybar),  ybar = mean_j y_j
  //   (every sample is pulled towards the minibatch's MEAN target). loss_mode 1 (not the reference): the per-sample form,
  //   loss = mean_i (q_i - y_i)^2, dL/dq_i = (2 / B) (q_i - y_i).
  float sq = 0.0f;
  if (t < LB) {  // (exactly wave 0: the wave reduction below runs with all 64 lanes)
    float g = 0.0f, target = 0.0f, qsa = 0.0f;
    if (t < B) {
      const float nq = fmaxf(fmaxf(L.tq[t * 4], L.tq[t * 4 + 1]), fmaxf(L.tq[t * 4 + 2], L.tq[t * 4 + 3]));
      const float discount = HYPER ? L.scratch[18] : a.discount;
      target = discount * (L.term[t] ? 0.0f : nq) + L.rew[t];
      qsa = L.q[t * 4 + L.act[t]];
    }
    if (a.loss_mode == 0) {
      const float ybar = __ockl_wfred_add_f32(target) / (float)B;  // (lanes >= B hold 0)
      if (t < B) {
        const float d = qsa - ybar, e = target - ybar;
        sq = fmaf(d, d, e * e);
        g = 2.0f * d / (float)B;
      }
    } else if (t < B) {
      const float d = qsa - target;
      sq = d * d;
      g = 2.0f * d / (float)B;
    }
    L.y[t] = g;
  }
  const float loss = block_sum(sq, L.scratch) / (float)B;  // (has barriers: y[] is visible afterwards)
  if (t < LB * 4) L.q[t] = ((t & 3) == L.act[t >> 2]) ? L.y[t >> 2] : 0.0f;  // q now holds dL/dq
  __syncthreads();
  SGK_STAMP(10);

  // ---- backward; every lane keeps the gradients of the parameters it owns in registers ----------------------------
  // dL/dh2 = relu'(h2) * (dq W3) -> C   (dense_layer with K = 4, "wt" = W3 [4][H])
  dense_layer<4, H>(L.q, 4, L.w3, nullptr, L.C, false, L.Bq);
  // W3 [4][H] on the matrix cores: wave w < MT takes the 16 columns k = 16 w .. of dq^T h2 (A = dq [b][4]: the tile's rows
  // 4 .. 15 are neighbouring samples' values and are dropped); the lanes of group 0 hold the four actions of column k.
  // b3 = column sums of dq: wave MT, lane 0 holds all four.
  f4 gw3 = {0.0f, 0.0f, 0.0f, 0.0f}, gb3 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (wave < MT) gw3 = weight_grad_mfma(L.q, 4, 0, L.Bq, H, 16 * wave, lane);
  else if (wave == MT) gb3 = column_sum_mfma(L.q, 4, 0, lane);
  const bool own_w3 = wave < MT && grp == 0 && 16 * wave + col < H;
  const bool own_b3 = wave == MT && lane == 0;
  if (!own_w3) gw3 = (f4){0.0f, 0.0f, 0.0f, 0.0f};
  if (!own_b3) gb3 = (f4){0.0f, 0.0f, 0.0f, 0.0f};
  __syncthreads();
  SGK_STAMP(11);
  // dL/dh1 = relu'(h1) * (dh2 W2) -> D   ("wt" = W2 as it is)
  dense_layer<H, H, weight_stride(H)>(L.C, H, L.ST, nullptr, L.D, false, L.A);
  // W2 [H][H] in 16 x 16 MFMA tiles dealt round-robin to the 16 waves (tile = (neuron tile, input tile)); the gradients stay in
  // registers, TRANSPOSED in the C layout (weight_grad_mfma_t): lane (col, grp), register r <-> dW2[j0 + col][k0 + 4 grp + r], four
  // consecutive elements of a row of W2. MT more tiles are b2's column sums of dL/dh2 (rows j0 + 4 grp + r, the same in every
  // column: the lanes of column 0 own them).
  constexpr int T2 = MT * MT + MT, T1 = MT * KT1 + MT;
  constexpr int N2 = (T2 + LWG / 64 - 1) / (LWG / 64), N1 = (T1 + LWG / 64 - 1) / (LWG / 64);  // tiles per wave
  f4 gw2[N2];
#pragma unroll
  for (int i = 0; i < N2; ++i) {
    const int tile = wave + i * (LWG / 64);
    gw2[i] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    if (tile < MT * MT) gw2[i] = weight_grad_mfma_t(L.C, H, 16 * (tile / MT), L.A, H, 16 * (tile % MT), lane);
    else if (tile < T2) gw2[i] = column_sum_mfma(L.C, H, 16 * (tile - MT * MT), lane);
  }
  __syncthreads();
  SGK_STAMP(12);
  // W1 [H][K0] the same way (columns = board cells; cells >= K0 of the last tile are computed from what lies behind the
  // row in LDS and dropped) -- transposed like W2 where a row's quads are 16-byte aligned (K0 % 4 == 0), else in the plain C layout
  // (register r <-> dW1[j0 + 4 grp + r][k0 + col]) --, then b1's column sums of dL/dh1
  constexpr bool W1T = (K0 % 4) == 0;
  f4 gw1[N1];
#pragma unroll
  for (int i = 0; i < N1; ++i) {
    const int tile = wave + i * (LWG / 64);
    gw1[i] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    if (tile < MT * KT1)
      gw1[i] = W1T ? weight_grad_mfma_t(L.D, H, 16 * (tile / KT1), L.S, KP, 16 * (tile % KT1), lane)
                   : weight_grad_mfma(L.D, H, 16 * (tile / KT1), L.S, KP, 16 * (tile % KT1), lane);
    else if (tile < T1) gw1[i] = column_sum_mfma(L.D, H, 16 * (tile - MT * KT1), lane);
  }
  // ---- clip_grad_norm_(max_norm): coefficient from the global 2-norm of all gradients -----------------------------
  float ss = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) ss = fmaf(gw3[c], gw3[c], fmaf(gb3[c], gb3[c], ss));
#pragma unroll
  for (int i = 0; i < N2; ++i) {
    const int tile = wave + i * (LWG / 64);
    const bool bias = tile >= MT * MT;
    // a weight tile's lane holds (row j0 + col, columns k0 + 4 grp + r); a bias tile's (rows j0 + 4 grp + r), counted once, in column 0
    const int j = 16 * (bias ? tile - MT * MT : tile / MT) + (bias ? 4 * grp : col), k = bias ? 0 : 16 * (tile % MT) + 4 * grp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // rows / columns past H belong to no parameter
      const bool live = tile < T2 && (bias ? (j + r < H && col == 0) : (j < H && k + r < H));
      gw2[i][r] = live ? gw2[i][r] : 0.0f;
      ss = fmaf(gw2[i][r], gw2[i][r], ss);
    }
  }
#pragma unroll
  for (int i = 0; i < N1; ++i) {
    const int tile = wave + i * (LWG / 64);
    const bool bias = tile >= MT * KT1;
    const bool tr = W1T && !bias;  // transposed ownership
    const int j = 16 * (bias ? tile - MT * KT1 : tile / KT1) + (tr ? col : 4 * grp), k = bias ? 0 : 16 * (tile % KT1) + (tr ? 4 * grp : col);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool live = tile < T1 && (bias ? (j + r < H && col == 0) : tr ? (j < H && k + r < K0) : (j + r < H && k < K0));
      gw1[i][r] = live ? gw1[i][r] : 0.0f;
      ss = fmaf(gw1[i][r], gw1[i][r], ss);
    }
  }
  // ---- Adam (amsgrad) on the owned parameters; the transposed copies follow ---------------------------------------
  // A lane owns NQ "quads": four parameters of one tensor at a fixed stride -- a column piece of a weight tile (rows j .. j + 3 at
  // column k: the MFMA C layout), four consecutive bias elements, W3's four rows of a column, or b3. Their old values (w, m, v,
  // vmax) are requested QD - 1 quads AHEAD: the first ones before the norm's reduction, quad i + QD - 1 before quad i is updated
  // and stored. (Per quad in turn -- load, update, store, next -- the seven quads were seven dependent round trips.)
  constexpr int NQ = 1 + N2 + N1;
  struct QuadRef {
    float *w, *m, *v, *x, *wt;  // tensor, Adam state, and where the quad goes in the transposed copy (null: none)
    int e0, stride, wt_stride;  // stride 1: four consecutive, 16-byte aligned elements
    bool on;
    int flat;                   // the tensor's offset in the flat parameter vector (ParamMap)
  };
  using PM = ParamMap<K0, H>;
  auto quad_ref = [&](int i) -> QuadRef {
    QuadRef r{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 1, false, 0};
    if (i == 0) {
      if (own_w3) { const int k = 16 * wave + col; const uint32_t o = mo.w3(); r = QuadRef{a.w3 + o, a.m[4] + o, a.v[4] + o, a.vmax[4] + o, a.w3t + o + 4 * k, k, H, 1, true, PM::o_w3}; }
      else if (own_b3) { const uint32_t o = mo.b3(); r = QuadRef{a.b3 + o, a.m[5] + o, a.v[5] + o, a.vmax[5] + o, nullptr, 0, 1, 1, true, PM::o_b3}; }
    } else if (i <= N2) {
      const int tile = wave + (i - 1) * (LWG / 64);
      if (tile < MT * MT) {
        const int j = 16 * (tile / MT) + col, k = 16 * (tile % MT) + 4 * grp;  // H % 4 == 0: the four columns k .. k + 3 are all inside
        const uint32_t o = mo.w2();
        if (j < H && k < H) r = QuadRef{a.w2 + o, a.m[2] + o, a.v[2] + o, a.vmax[2] + o, a.w2t + o + (size_t)k * H + j, j * H + k, 1, H, true, PM::o_w2};
      } else if (tile < T2) {
        const int jb = 16 * (tile - MT * MT) + 4 * grp;
        const uint32_t o = mo.b();
        if (col == 0 && jb < H) r = QuadRef{a.b2 + o, a.m[3] + o, a.v[3] + o, a.vmax[3] + o, nullptr, jb, 1, 1, true, PM::o_b2};
      }
    } else {
      const int tile = wave + (i - 1 - N2) * (LWG / 64);
      if (tile < MT * KT1) {
        if (W1T) {
          const int j = 16 * (tile / KT1) + col, k = 16 * (tile % KT1) + 4 * grp;
          const uint32_t o = mo.w1();
          if (j < H && k < K0) r = QuadRef{a.w1 + o, a.m[0] + o, a.v[0] + o, a.vmax[0] + o, a.w1t + o + (size_t)k * H + j, j * K0 + k, 1, H, true, PM::o_w1};
        } else {
          const int j = 16 * (tile / KT1) + 4 * grp, k = 16 * (tile % KT1) + col;
          const uint32_t o = mo.w1();
          if (j < H && k < K0) r = QuadRef{a.w1 + o, a.m[0] + o, a.v[0] + o, a.vmax[0] + o, a.w1t + o + (size_t)k * H + j, j * K0 + k, K0, 1, true, PM::o_w1};
        }
      } else if (tile < T1) {
        const int jb = 16 * (tile - MT * KT1) + 4 * grp;
        const uint32_t o = mo.b();
        if (col == 0 && jb < H) r = QuadRef{a.b1 + o, a.m[1] + o, a.v[1] + o, a.vmax[1] + o, nullptr, jb, 1, 1, true, PM::o_b1};
      }
    }
    return r;
  };
  struct QuadVals { f4 w, m, v, x; };
  auto quad_request = [&](QuadVals &q, const QuadRef &r) {
    q.w = q.m = q.v = q.x = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    if (r.on) {
      if (r.stride == 1) {
        q.w = *reinterpret_cast<const f4 *>(r.w + r.e0); q.m = *reinterpret_cast<const f4 *>(r.m + r.e0);
        q.v = *reinterpret_cast<const f4 *>(r.v + r.e0); q.x = *reinterpret_cast<const f4 *>(r.x + r.e0);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int e = r.e0 + c * r.stride;
          q.w[c] = r.w[e]; q.m[c] = r.m[e]; q.v[c] = r.v[e]; q.x[c] = r.x[e];
        }
      }
    }
  };
  // (how far ahead: measured with one and with two quads ahead -- 10.0 and 9.0 us for the phase, the second at the price of register
  // spills -- so the trips are not what bounds it. With -DSGK_LEARN_TIMELINE_ADAM wave 0 takes 0.5-1.3 us per quad whatever the
  // distance and then waits 2.9 us at the barrier for the other waves: the phase moves ~500 KB (13.9 k parameters x 4 tensors in, 5
  // out, padded tiles and 4-lane bias quads at full instruction cost) through ONE CU's 64 B/clk vector-memory path at ~40 % of
  // that rate. What would shorten it is more CUs, and a second workgroup costs a grid barrier: EXPERIMENTS R6.4.)
  constexpr int QD = 2;
  if (a.adam_scratch) {  // (wave-uniform) two launches: the gradient leaves here, dqn_adam_kernel applies it
    float *const scratch = a.adam_scratch + mb * (size_t)a.scratch_stride;  // this member's slice of the workspace
    float *gout = scratch + sizeof(AdamHeader) / sizeof(float);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const QuadRef r = quad_ref(i);
      const f4 g = i == 0 ? (own_w3 ? gw3 : gb3) : (i <= N2 ? gw2[i <= N2 ? i - 1 : 0] : gw1[i > N2 ? i - 1 - N2 : 0]);
      if (r.on) {
        if (r.stride == 1) *reinterpret_cast<f4 *>(gout + r.flat + r.e0) = g;
        else {
#pragma unroll
          for (int c = 0; c < 4; ++c) gout[r.flat + r.e0 + c * r.stride] = g[c];
        }
      }
    }
    const float norm2 = sqrtf(block_sum(ss, L.scratch));
    if (t == 0) {
      AdamHeader hd;
      hd.coef = fminf(a.max_norm / (norm2 + 1e-6f), 1.0f);
      hd.lr_bc1 = L.scratch[16];
      hd.inv_bc2_sqrt = L.scratch[17];
      hd.pad = 0.0f;
      *reinterpret_cast<AdamHeader *>(scratch) = hd;
      a.step[mb] = step0 + 1;
      if (a.loss_out) a.loss_out[mb] = loss;
    }
    SGK_STAMP(13);
    return;
  }
  QuadVals qv[QD];
#pragma unroll
  for (int i = 0; i < QD - 1 && i < NQ; ++i) quad_request(qv[i], quad_ref(i));
  const float norm = sqrtf(block_sum(ss, L.scratch));
  SGK_STAMP(13);
  const float coef = fminf(a.max_norm / (norm + 1e-6f), 1.0f);
  AdamCoef ac;
  ac.lr_bc1 = L.scratch[16];  // (the bias corrections: computed at entry)
  ac.inv_bc2_sqrt = L.scratch[17];
  ac.beta1 = a.beta1; ac.beta2 = a.beta2; ac.eps = a.eps;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    if (i + QD - 1 < NQ) quad_request(qv[(i + QD - 1) % QD], quad_ref(i + QD - 1));
#ifdef SGK_LEARN_TIMELINE_ADAM
    SGK_STAMP(14 + i);
#endif
    const QuadRef r = quad_ref(i);
    QuadVals &q = qv[i % QD];
    const f4 g = i == 0 ? (own_w3 ? gw3 : gb3) : (i <= N2 ? gw2[i <= N2 ? i - 1 : 0] : gw1[i > N2 ? i - 1 - N2 : 0]);
    if (r.on) {
      f4 nw, nm, nv, nx;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float m = q.m[c], v = q.v[c], x = q.x[c];
        nw[c] = adam_scalar(q.w[c], m, v, x, g[c] * coef, ac);
        nm[c] = m; nv[c] = v; nx[c] = x;
      }
      if (r.stride == 1) {
        *reinterpret_cast<f4 *>(r.w + r.e0) = nw; *reinterpret_cast<f4 *>(r.m + r.e0) = nm;
        *reinterpret_cast<f4 *>(r.v + r.e0) = nv; *reinterpret_cast<f4 *>(r.x + r.e0) = nx;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int e = r.e0 + c * r.stride;
          r.w[e] = nw[c]; r.m[e] = nm[c]; r.v[e] = nv[c]; r.x[e] = nx[c];
        }
      }
      if (r.wt) {
        if (r.wt_stride == 1) *reinterpret_cast<f4 *>(r.wt) = nw;
        else {
#pragma unroll
          for (int c = 0; c < 4; ++c) r.wt[(size_t)c * r.wt_stride] = nw[c];
        }
      }
    }
  }
  if (t == 0) {
    a.step[mb] = step0 + 1;
    if (a.loss_out) a.loss_out[mb] = loss;
  }
#ifdef SGK_LEARN_TIMELINE
#ifdef SGK_LEARN_TIMELINE_ADAM
  SGK_STAMP(14 + NQ);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  SGK_STAMP(15 + NQ);
  __syncthreads();
  SGK_STAMP(16 + NQ);
#else
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's updates are out
  __syncthreads();
  SGK_STAMP(14);
#endif
#endif
}

// Adam(amsgrad) + the transposed copies, one lane per parameter (the second launch of sgk_dqn_sgd_step: see AdamHeader above)
template <int K0, int H>
__device__ __forceinline__ void adam_body(const LearnArgs &a, int vblock, size_t mb = 0) {
  using PM = ParamMap<K0, H>;
  const MemberOffsets<K0, H> mo{(uint32_t)mb};
  const float *scratch = a.adam_scratch + mb * (size_t)a.scratch_stride;
  const AdamHeader hd = *reinterpret_cast<const AdamHeader *>(scratch);
  const float *g = scratch + sizeof(AdamHeader) / sizeof(float);
  AdamCoef ac;
  ac.lr_bc1 = hd.lr_bc1;
  ac.inv_bc2_sqrt = hd.inv_bc2_sqrt;
  ac.beta1 = a.beta1; ac.beta2 = a.beta2; ac.eps = a.eps;
  const int e = (int)(vblock * 256 + threadIdx.x);
  if (e >= PM::P) return;
  const int ten = e < PM::o_b1 ? 0 : e < PM::o_w2 ? 1 : e < PM::o_b2 ? 2 : e < PM::o_w3 ? 3 : e < PM::o_b3 ? 4 : 5;
  const int off = ten == 0 ? PM::o_w1 : ten == 1 ? PM::o_b1 : ten == 2 ? PM::o_w2 : ten == 3 ? PM::o_b2 : ten == 4 ? PM::o_w3 : PM::o_b3;
  float *wp = ten == 0 ? a.w1 : ten == 1 ? a.b1 : ten == 2 ? a.w2 : ten == 3 ? a.b2 : ten == 4 ? a.w3 : a.b3;
  const size_t le = mo.tensor(ten) + (size_t)(e - off);  // (the member's slice of the tensor, then the element)
  float m = a.m[ten][le], v = a.v[ten][le], x = a.vmax[ten][le];
  const float nw = adam_scalar(wp[le], m, v, x, g[e] * hd.coef, ac);
  wp[le] = nw;
  a.m[ten][le] = m; a.v[ten][le] = v; a.vmax[ten][le] = x;
  // the transposed copies the policy kernels (W1^T, W3^T) and the next step's forward (W2^T) read
  const int l = e - off;
  if (ten == 0) { const int j = l / K0, k = l - j * K0; a.w1t[mo.w1() + (size_t)k * H + j] = nw; }
  else if (ten == 2) { const int j = l / H, k = l - j * H; a.w2t[mo.w2() + (size_t)k * H + j] = nw; }
  else if (ten == 4) { const int ai = l / H, k = l - ai * H; a.w3t[mo.w3() + 4 * k + ai] = nw; }
}

template <int K0, int H, bool MEMBERS = false>  // (MEMBERS as for dqn_sgd_kernel: false is the launch of one member's NB workgroups)
__global__ __launch_bounds__(256) void dqn_adam_kernel(LearnArgs a) {
  constexpr int NB = (ParamMap<K0, H>::P + 255) / 256;  // the grid is n_members x NB: workgroup -> (member, block)
  const int mb = MEMBERS ? (int)blockIdx.x / NB : 0;
  adam_body<K0, H>(a, (int)blockIdx.x - mb * NB, (size_t)mb);
}

// Adam AND the lockstep step's last launch -- reset_done + the next transitions' states into the replay ring (sgk_reset_done_store) --
// in one grid (sgk_dqn_sgd_step_reset_store): the two are independent (the reset neither reads the weights nor the minibatch, and the
// SGD kernel before this launch has finished sampling the ring), each alone is a 5 us launch that leaves most of the chip idle. The
// first adam_blocks workgroups run Adam, the others the reset kernel's body over their own virtual grid.
struct ResetStoreArgs {
  const SgkRules *rules;
  uint64_t *state;
  int8_t *boards;
  int32_t *n_resets;
  const double *aux;
  int64_t n;
  uint64_t seed, env_base;
  int32_t mode_flags;
  StepStore st;
};
template <int H, int ENV, int LAYOUT>
__global__ __launch_bounds__(256) void dqn_adam_reset_kernel(LearnArgs a, int adam_blocks, ResetStoreArgs r) {
  static_assert(WG == 256, "the reset body's workgroup");
  if ((int)blockIdx.x < adam_blocks) {  // (workgroup-uniform)
    adam_body<Geom<ENV>::NC, H>(a, (int)blockIdx.x);
  } else {
    reset_body<ENV, LAYOUT, true>(r.rules, r.state, r.boards, nullptr, r.mode_flags, r.n, r.seed, r.env_base, r.n_resets, r.aux, r.st,
                                  (int)blockIdx.x - adam_blocks, (int)gridDim.x - adam_blocks);
  }
}

// ------------------------------------------------------------------------------------------------
// PPOBaseAgent.learn (reference policy_base.py:64-131) for PPOMLPAgent's default topology, ALL epochs in one launch: per
// epoch a minibatch of rows drawn with replacement from the gathered rollout, the current network (trunk, actor, critic)
// and the old policy (trunk, actor) forward, the clipped surrogate with batch-normalised advantages, critic MSE and entropy
// bonus, the backward pass (including the path of the policy loss into the critic through the normalised advantage, which
// the reference's autograd graph has) and Adam. Same structure as dqn_sgd_kernel: one workgroup, activations in LDS, weight
// matrices staged per phase, dense layers and weight gradients on fp32 MFMA.
// The grid is one workgroup per MEMBER (sgk_ppo_epochs_members; one member = sgk_ppo_epochs): every tensor below but the rollout is
// stacked [n_members][...] and the pointers address member 0; workgroup m moves them to its own slice, draws its rows from its own
// trajectories m * E .. (m + 1) * E - 1 (rows stay global: t * N + trajectory) with its own Philox key, and runs the body as it is.
// The workgroup fills a CU's LDS, so the members run one per CU.
// ------------------------------------------------------------------------------------------------
struct PpoArgs {
  // rollout: states int8 [T][N][K0], actions uint8 [T][N], returns float [N][T], lengths int32 [N]
  const int8_t *states;
  const uint8_t *actions;
  const float *returns;
  const int32_t *lengths;
  int32_t T;
  int64_t N;
  int64_t E;  // trajectories per member (N with one member)
  // current network (torch layouts), updated in place; transposed trunk copies kept current; Adam state per tensor
  float *w1, *b1, *w2, *b2, *wa, *ba, *wc, *bc;  // wa [4][H], ba [4], wc [1][H], bc [1]
  float *w1t, *w2t;
  float *m[8], *v[8];  // order: w1, b1, w2, b2, wa, ba, wc, bc
  // old policy: transposed trunk weights, actor as it is
  const float *ow1t, *ob1, *ow2t, *ob2, *owa, *oba;
  long long *step;   // Adam step counter (device), one per member; also the key of the minibatch draws
  float *stats_out;  // [n_epochs][3] per member: policy loss, value loss, entropy; or null
  const long long *rows;  // [n_epochs][batch] per member: rows t * N + env to use instead of the random draws; or null
  long long *rows_out;    // [n_epochs][batch] per member: the rows each epoch used; or null
  int32_t batch, n_epochs;
  uint64_t seed;
  const uint64_t *member_keys;  // [n_members] Philox keys of the members' draws; null: `seed` for every member
  float lr, beta1, beta2, eps, clipping, critic_coeff, entropy_bonus;
  // sgk_ppo_epochs_members_hyper (the HYPER instantiation only): [n_members], member m's lr / clipping / critic_coeff / entropy_bonus
  const PpoMemberHyper *member_hyper;
};

struct PpoLds {
  float *A, *Bq, *C, *D, *ST, *wh, *owa, *b1, *b2, *ob1, *ob2, *bh, *oba, *out, *oout, *dout, *ret, *scratch;
  int8_t *S;
  int *act;
};

template <int KP, int H>
__device__ __forceinline__ PpoLds carve_ppo(unsigned char *base) {
  PpoLds L;
  float *f = reinterpret_cast<float *>(base);
  L.A = f; f += LB * H;      // current hidden 1
  L.Bq = f; f += LB * H;     // current hidden 2
  L.C = f; f += LB * H;      // old hidden 1, then dL/dh2
  L.D = f; f += LB * H;      // old hidden 2, then dL/dh1
  L.ST = f; f += H * weight_stride(H);  // the weight matrix of the running phase (padded rows)
  L.wh = f; f += 8 * H;      // current heads: rows 0..3 actor, row 4 critic, rows 5..7 zero
  L.owa = f; f += 4 * H;     // old actor
  L.b1 = f; f += H;
  L.b2 = f; f += H;
  L.ob1 = f; f += H;
  L.ob2 = f; f += H;
  L.bh = f; f += 8;          // actor biases, critic bias, zeros
  L.oba = f; f += 4;
  L.out = f; f += LB * 8;    // current logits [0..3], value [4]
  L.oout = f; f += LB * 4;   // old logits
  L.dout = f; f += LB * 8;   // dL/d(logits, value), zero-padded to 8
  L.ret = f; f += LB;
  L.scratch = f; f += 32;
  L.act = reinterpret_cast<int *>(f); f += LB;
  L.S = reinterpret_cast<int8_t *>(f);
  return L;
}

constexpr size_t ppo_lds_bytes(int KP, int H) {
  return sizeof(float) * ((size_t)4 * LB * H + (size_t)H * weight_stride(H) + 12 * H + 4 * H + 12 + LB * 8 + LB * 4 + LB * 8 + LB + 32 + LB) +
         (size_t)LB * KP + 64;
}

// heads: out[b][o] = bh[o] + sum_k h[b][k] * wh[o][k] for o < NOUT (all LDS): one lane per (b, o)
template <int NOUT, int OS>
__device__ __forceinline__ void heads_forward(const float *h, int H, const float *wh, const float *bh, float *out) {
  if (threadIdx.x < LB * NOUT) {
    const int b = threadIdx.x / NOUT, o = threadIdx.x % NOUT;
    float acc = bh[o];
    for (int k0 = 0; k0 < H; k0 += 4) {
      const f4 w = *reinterpret_cast<const f4 *>(wh + o * H + k0);
      const f4 x = *reinterpret_cast<const f4 *>(h + b * H + k0);
      acc = fmaf(x[0], w[0], acc);
      acc = fmaf(x[1], w[1], acc);
      acc = fmaf(x[2], w[2], acc);
      acc = fmaf(x[3], w[3], acc);
    }
    out[b * OS + o] = acc;
  }
}

__device__ __forceinline__ float adam_plain(float p, float &m, float &v, float g, const AdamCoef &c) {
  m = m + (1.0f - c.beta1) * (g - m);
  v = c.beta2 * v + (1.0f - c.beta2) * g * g;
  return p - c.lr_bc1 * (m * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) * c.inv_bc2_sqrt + c.eps));  // (one-ulp sqrt / rcp: adam_scalar)
}

// HYPER = true (sgk_ppo_epochs_members_hyper): workgroup m reads lr, clipping, critic_coeff and entropy_bonus from its element of
// a.member_hyper instead of `a`, converted with the host's (float) cast -- ONE 32-byte load at entry, where the member's offsets are
// formed, parked in LDS (scratch[18 .. 21]: the epoch loop's first barrier publishes them) so that no register lives across the
// epochs for them: the kernel sits at its 128-VGPR budget.
template <int K0, int H, bool HYPER = false>
__global__ __launch_bounds__(LWG) void ppo_epochs_kernel(PpoArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char learn_smem[];
  constexpr int KP = (K0 + 3) & ~3;
  const PpoLds L = carve_ppo<KP, H>(learn_smem);
  const int t0 = threadIdx.x, B = a.batch;
  constexpr int MT = (H + 15) / 16, KT1 = (K0 + 15) / 16;
  constexpr int T2 = MT * MT + MT, T1 = MT * KT1 + MT;  // weight tiles + the bias tiles (column sums)
  constexpr int N2 = (T2 + LWG / 64 - 1) / (LWG / 64), N1 = (T1 + LWG / 64 - 1) / (LWG / 64);
  {  // this member's slice of every stacked tensor (wave-uniform address arithmetic, once)
    const size_t mb = blockIdx.x;
    const size_t sz[8] = {(size_t)H * K0, (size_t)H, (size_t)H * H, (size_t)H, (size_t)4 * H, 4, (size_t)H, 1};
    a.w1 += mb * sz[0]; a.b1 += mb * sz[1]; a.w2 += mb * sz[2]; a.b2 += mb * sz[3];
    a.wa += mb * sz[4]; a.ba += mb * sz[5]; a.wc += mb * sz[6]; a.bc += mb * sz[7];
    a.w1t += mb * sz[0]; a.w2t += mb * sz[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) { a.m[i] += mb * sz[i]; a.v[i] += mb * sz[i]; }
    a.ow1t += mb * sz[0]; a.ob1 += mb * sz[1]; a.ow2t += mb * sz[2]; a.ob2 += mb * sz[3]; a.owa += mb * sz[4]; a.oba += mb * sz[5];
    a.step += mb;
    const size_t per_epoch = mb * (size_t)a.n_epochs;
    if (a.stats_out) a.stats_out += per_epoch * 3;
    if (a.rows) a.rows += per_epoch * (size_t)a.batch;
    if (a.rows_out) a.rows_out += per_epoch * (size_t)a.batch;
    if (a.member_keys) a.seed = a.member_keys[mb];
    if constexpr (HYPER) {
      if (t0 == 0) {
        const PpoMemberHyper hp = a.member_hyper[mb];
        L.scratch[18] = (float)hp.lr; L.scratch[19] = (float)hp.clipping;
        L.scratch[20] = (float)hp.critic_coeff; L.scratch[21] = (float)hp.entropy_bonus;
      }
    }
  }
  const long long traj0 = (long long)blockIdx.x * a.E;  // this member's first trajectory
  const long long step0 = *a.step;
  {
    const int t = t0;
  // the old policy does not change during the call: its small tensors are staged once
  stage(L.owa, a.owa, 4 * H);
  stage(L.ob1, a.ob1, H);
  stage(L.ob2, a.ob2, H);
  if (t < 4) L.oba[t] = a.oba[t];
  for (int i = t; i < 3 * H; i += LWG) L.wh[5 * H + i] = 0.0f;  // rows 5..7 of the padded head matrix
  if (t < 3) L.bh[5 + t] = 0.0f;
  }

  // The rows of an epoch depend only on (seed, Adam step, lengths): they are drawn one epoch AHEAD -- behind the backward pass,
  // in front of the Adam stores -- so that the three dependent memory round trips (lengths, then action / return, then the
  // board gather's addresses) are off the critical path. `t`, `lane`: this lane's ids (laundered per epoch, see below).
  auto draw_rows = [&](int e_ix, long long e_step, int t, int lane) {
  // ---- minibatch: a row = a (t, env) pair inside that env's episode, uniform with replacement. Each sample tries 16
  // candidates per round (16 lanes), the first valid one in lane order wins; another round only if all 16 miss. ----
  {
    const int b = t >> 4, c = t & 15;  // 64 samples x 16 candidate lanes
    int tt = 0;
    long long nn = 0;
    bool found = a.rows != nullptr;
    if (found && b < B) {
      long long row = a.rows[(long long)e_ix * B + b];
      row = row < 0 ? 0 : (row >= (long long)a.T * a.N ? (long long)a.T * a.N - 1 : row);  // a bad row must not leave the rollout
      tt = (int)(row / a.N);
      nn = row - (long long)tt * a.N;
    }
    for (int round = 0; round < 64 && !found; ++round) {
      uint32_t x[4];
      philox4x32_10((uint32_t)(b * 16 + c), (uint32_t)round, (uint32_t)e_step, 5u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), x);
      const long long n_c = traj0 + (long long)__umul64hi(((unsigned long long)x[0] << 32) | x[1], (unsigned long long)a.E);
      const int t_c = (int)__umulhi(x[2], (uint32_t)a.T);
      const bool ok = t_c < a.lengths[n_c];
      const unsigned long long mask = __ballot(ok);
      const unsigned int mine = (unsigned int)((mask >> (lane & 48)) & 0xffffull);  // this sample's 16 candidate lanes
      if (mine) {
        const int win = (lane & 48) + __ffs(mine) - 1;
        tt = __shfl(t_c, win, 64);
        nn = __shfl((int)n_c, win, 64);  // N < 2^31 (checked by the launcher)
        found = true;
      }
    }
    if (c == 0) {
      const long long row = (long long)tt * a.N + nn;
      L.act[b] = b < B ? (int)(a.actions[row] & 3) : 0;
      L.ret[b] = b < B ? a.returns[nn * a.T + tt] : 0.0f;
      reinterpret_cast<long long *>(L.oout)[b] = row;  // parked for the gather at the top of that epoch (oout is free until then)
      if (a.rows_out && b < B) a.rows_out[(long long)e_ix * B + b] = row;
    }
  }
  };
  draw_rows(0, step0, t0, t0 & 63);

  for (int epoch = 0; epoch < a.n_epochs; ++epoch) {
    const long long step = step0 + epoch;  // Adam steps done before this epoch; keys the minibatch draws
    // the lane id is re-derived through an opaque move every epoch: with a loop-invariant id the compiler hoists the ~100
    // per-lane 64-bit addresses of the Adam phase out of the loop and keeps them live across it (261 VGPRs spilled)
    int t = t0;
    asm volatile("" : "+v"(t));
    const int lane = t & 63, wave = t >> 6, col = lane & 15, grp = lane >> 4;
    __syncthreads();                       // the previous epoch's update is complete before anything of it is re-read
    stage_rows<H>(L.ST, a.ow1t, K0);
    stage(L.wh, a.wa, 4 * H);
    stage(L.wh + 4 * H, a.wc, H);
    stage(L.b1, a.b1, H);
    stage(L.b2, a.b2, H);
    if (t < 4) L.bh[t] = a.ba[t];
    if (t == 4) L.bh[4] = a.bc[0];
    __syncthreads();
    for (int i = t; i < LB * KP; i += LWG) {
      const int b = i / KP, k = i - b * KP;
      const long long row = reinterpret_cast<const long long *>(L.oout)[b];
      L.S[i] = (b < B && k < K0) ? a.states[row * K0 + k] : (int8_t)0;
    }
    __syncthreads();
    // ---- old policy, then current network, on the same states ----
    dense_layer<K0, H, weight_stride(H)>(L.S, KP, L.ST, L.ob1, L.C, true, nullptr);
    __syncthreads();
    stage_rows<H>(L.ST, a.ow2t, H);
    __syncthreads();
    dense_layer<H, H, weight_stride(H)>(L.C, H, L.ST, L.ob2, L.D, true, nullptr);
    __syncthreads();
    heads_forward<4, 4>(L.D, H, L.owa, L.oba, L.oout);
    stage_rows<H>(L.ST, a.w1t, K0);
    __syncthreads();
    dense_layer<K0, H, weight_stride(H)>(L.S, KP, L.ST, L.b1, L.A, true, nullptr);
    __syncthreads();
    stage_rows<H>(L.ST, a.w2t, H);
    __syncthreads();
    dense_layer<H, H, weight_stride(H)>(L.A, H, L.ST, L.b2, L.Bq, true, nullptr);
    __syncthreads();
    heads_forward<5, 8>(L.Bq, H, L.wh, L.bh, L.out);
    stage_rows<H>(L.ST, a.w2, H);  // W2 as it is, for the back-propagation
    __syncthreads();
    // ---- losses and dL/d(logits, value): the 64 samples are the 64 lanes of wave 0, batch statistics by wave reductions ----
    if (wave == 0) {
      const int b = lane;
      const bool live = b < B;
      const float invB = 1.0f / (float)B;
      float l[4], lo[4], p[4], logp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { l[k] = L.out[b * 8 + k]; lo[k] = L.oout[b * 4 + k]; }
      const float v = L.out[b * 8 + 4], r = L.ret[b];
      const int ac = L.act[b];
      const float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3])), mxo = fmaxf(fmaxf(lo[0], lo[1]), fmaxf(lo[2], lo[3]));
      const float lse = mx + logf(expf(l[0] - mx) + expf(l[1] - mx) + expf(l[2] - mx) + expf(l[3] - mx));
      const float lseo = mxo + logf(expf(lo[0] - mxo) + expf(lo[1] - mxo) + expf(lo[2] - mxo) + expf(lo[3] - mxo));
      float ent = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) { logp[k] = l[k] - lse; p[k] = expf(logp[k]); ent -= p[k] * logp[k]; }
      const float logp_a = ac == 0 ? logp[0] : ac == 1 ? logp[1] : ac == 2 ? logp[2] : logp[3];
      const float lo_a = (ac == 0 ? lo[0] : ac == 1 ? lo[1] : ac == 2 ? lo[2] : lo[3]) - lseo;
      const float ratio = expf(logp_a - lo_a);
      // advantages normalised over the minibatch (unbiased std, as torch.std)
      const float adv = live ? r - v : 0.0f;
      const float mu = __ockl_wfred_add_f32(adv) * invB;
      const float dev = live ? adv - mu : 0.0f;
      const float sigma = sqrtf(__ockl_wfred_add_f32(dev * dev) / (float)(B - 1));
      const float advn = dev / sigma;
      const float clipping = HYPER ? L.scratch[19] : a.clipping, critic_coeff = HYPER ? L.scratch[20] : a.critic_coeff;
      const float entropy_bonus = HYPER ? L.scratch[21] : a.entropy_bonus;
      const float lo_c = 1.0f - clipping, hi_c = 1.0f + clipping;
      const float rc = fminf(fmaxf(ratio, lo_c), hi_c);
      const float s1 = advn * ratio, s2 = advn * rc;
      const float w1 = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f), w2 = 1.0f - w1;  // torch.min's gradient: halves on a tie
      const float inrange = (ratio >= lo_c && ratio <= hi_c) ? 1.0f : 0.0f;
      const float g_advn = live ? -invB * (w1 * ratio + w2 * rc) : 0.0f;
      const float g_ratio = live ? -invB * advn * (w1 + w2 * inrange) : 0.0f;
      const float g_logp = g_ratio * ratio;
      // back through the normalisation: dL/dadv_j = (g_j - mean g) / sigma - (adv_j - mu) * S / ((B - 1) sigma^3)
      const float gbar = __ockl_wfred_add_f32(g_advn) * invB;
      const float S = __ockl_wfred_add_f32(g_advn * dev);
      const float g_adv = live ? (g_advn - gbar) / sigma - dev * S / ((float)(B - 1) * sigma * sigma * sigma) : 0.0f;
      const float dv = live ? critic_coeff * 2.0f * (v - r) * invB - g_adv : 0.0f;
      float dl[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float onehot = k == ac ? 1.0f : 0.0f;
        dl[k] = live ? g_logp * (onehot - p[k]) + entropy_bonus * invB * p[k] * (logp[k] + ent) : 0.0f;
      }
      *reinterpret_cast<f4 *>(L.dout + b * 8) = (f4){dl[0], dl[1], dl[2], dl[3]};
      *reinterpret_cast<f4 *>(L.dout + b * 8 + 4) = (f4){dv, 0.0f, 0.0f, 0.0f};
      if (a.stats_out) {
        const float pl = -__ockl_wfred_add_f32(live ? fminf(s1, s2) : 0.0f) * invB;
        const float vl = __ockl_wfred_add_f32(live ? (v - r) * (v - r) : 0.0f) * invB;
        const float en = __ockl_wfred_add_f32(live ? ent : 0.0f) * invB;
        if (lane == 0) { a.stats_out[epoch * 3] = pl; a.stats_out[epoch * 3 + 1] = vl; a.stats_out[epoch * 3 + 2] = en; }
      }
    }
    __syncthreads();
    // ---- backward ----
    dense_layer<8, H>(L.dout, 8, L.wh, nullptr, L.C, false, L.Bq);  // dL/dh2 = relu'(h2) * (dout W_heads) -> C
    // head weights [5][H] on the matrix cores: wave w < MT takes the columns k = 16 w ..; A = dout [b][8], so the tile's rows
    // 0..3 are the actor (registers of group 0), row 4 the critic (register 0 of group 1), rows 8..15 the next sample's values
    // (dropped). Head biases = column sums of dout: wave MT (lane 0: actor, lane 16: critic).
    f4 gh = {0.0f, 0.0f, 0.0f, 0.0f}, gbh = {0.0f, 0.0f, 0.0f, 0.0f};
    if (wave < MT) gh = weight_grad_mfma(L.dout, 8, 0, L.Bq, H, 16 * wave, lane);
    else if (wave == MT) gbh = column_sum_mfma(L.dout, 8, 0, lane);
    __syncthreads();
    dense_layer<H, H, weight_stride(H)>(L.C, H, L.ST, nullptr, L.D, false, L.A);  // dL/dh1 -> D
    // W2 tiles, then MT more tiles with b2's column sums of dL/dh2 (owned by the lanes of column 0); W1 / b1 the same way
    f4 gw2[N2];
#pragma unroll
    for (int i = 0; i < N2; ++i) {
      const int tile = wave + i * (LWG / 64);
      gw2[i] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
      if (tile < MT * MT) gw2[i] = weight_grad_mfma(L.C, H, 16 * (tile / MT), L.A, H, 16 * (tile % MT), lane);
      else if (tile < T2) gw2[i] = column_sum_mfma(L.C, H, 16 * (tile - MT * MT), lane);
    }
    __syncthreads();
    f4 gw1[N1];
#pragma unroll
    for (int i = 0; i < N1; ++i) {
      const int tile = wave + i * (LWG / 64);
      gw1[i] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
      if (tile < MT * KT1) gw1[i] = weight_grad_mfma(L.D, H, 16 * (tile / KT1), L.S, KP, 16 * (tile % KT1), lane);
      else if (tile < T1) gw1[i] = column_sum_mfma(L.D, H, 16 * (tile - MT * KT1), lane);
    }
    if (epoch + 1 < a.n_epochs) draw_rows(epoch + 1, step + 1, t, lane);  // act / ret / oout are free from here on
    // ---- Adam (torch defaults: no amsgrad, no gradient clipping) ----
    if (t == 0) {
      L.scratch[16] = (HYPER ? L.scratch[18] : a.lr) / (float)(1.0 - pow((double)a.beta1, (double)(step + 1)));
      L.scratch[17] = 1.0f / sqrtf((float)(1.0 - pow((double)a.beta2, (double)(step + 1))));
    }
    __syncthreads();
    AdamCoef ac;
    ac.lr_bc1 = L.scratch[16];
    ac.inv_bc2_sqrt = L.scratch[17];
    ac.beta1 = a.beta1; ac.beta2 = a.beta2; ac.eps = a.eps;
    if (wave < MT && 16 * wave + col < H) {
      const int k = 16 * wave + col;
      if (grp == 0) {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const int e = o * H + k;
          float m = a.m[4][e], v = a.v[4][e];
          a.wa[e] = adam_plain(a.wa[e], m, v, gh[o], ac);
          a.m[4][e] = m; a.v[4][e] = v;
        }
      } else if (grp == 1) {
        float m = a.m[6][k], v = a.v[6][k];
        a.wc[k] = adam_plain(a.wc[k], m, v, gh[0], ac);
        a.m[6][k] = m; a.v[6][k] = v;
      }
    } else if (wave == MT && lane == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float m = a.m[5][e], v = a.v[5][e];
        a.ba[e] = adam_plain(a.ba[e], m, v, gbh[e], ac);
        a.m[5][e] = m; a.v[5][e] = v;
      }
    } else if (wave == MT && lane == 16) {
      float m = a.m[7][0], v = a.v[7][0];
      a.bc[0] = adam_plain(a.bc[0], m, v, gbh[0], ac);
      a.m[7][0] = m; a.v[7][0] = v;
    }
#pragma unroll
    for (int i = 0; i < N2; ++i) {
      const int tile = wave + i * (LWG / 64);
      const int j = 16 * (tile / MT) + 4 * grp, k = 16 * (tile % MT) + col;
      if (tile >= MT * MT && tile < T2) {
        const int jb = 16 * (tile - MT * MT) + 4 * grp;
        if (col == 0 && jb < H) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float m = a.m[3][jb + r], v = a.v[3][jb + r];
            a.b2[jb + r] = adam_plain(a.b2[jb + r], m, v, gw2[i][r], ac);
            a.m[3][jb + r] = m; a.v[3][jb + r] = v;
          }
        }
      } else if (tile < MT * MT && j < H && k < H) {
        f4 nw;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = (j + r) * H + k;
          float m = a.m[2][e], v = a.v[2][e];
          nw[r] = adam_plain(a.w2[e], m, v, gw2[i][r], ac);
          a.w2[e] = nw[r]; a.m[2][e] = m; a.v[2][e] = v;
        }
        *reinterpret_cast<f4 *>(a.w2t + (size_t)k * H + j) = nw;
      }
    }
#pragma unroll
    for (int i = 0; i < N1; ++i) {
      const int tile = wave + i * (LWG / 64);
      const int j = 16 * (tile / KT1) + 4 * grp, k = 16 * (tile % KT1) + col;
      if (tile >= MT * KT1 && tile < T1) {
        const int jb = 16 * (tile - MT * KT1) + 4 * grp;
        if (col == 0 && jb < H) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float m = a.m[1][jb + r], v = a.v[1][jb + r];
            a.b1[jb + r] = adam_plain(a.b1[jb + r], m, v, gw1[i][r], ac);
            a.m[1][jb + r] = m; a.v[1][jb + r] = v;
          }
        }
      } else if (tile < MT * KT1 && j < H && k < K0) {
        f4 nw;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = (j + r) * K0 + k;
          float m = a.m[0][e], v = a.v[0][e];
          nw[r] = adam_plain(a.w1[e], m, v, gw1[i][r], ac);
          a.w1[e] = nw[r]; a.m[0][e] = m; a.v[0][e] = v;
        }
        *reinterpret_cast<f4 *>(a.w1t + (size_t)k * H + j) = nw;
      }
    }
    // no device-scope fence: the next epoch's staging loads are ordered behind these stores by the workgroup barrier at the top
    // of the loop (same CU, one L1), and nobody else reads the parameters before the kernel ends (it cost ~4 us per epoch)
  }
  __syncthreads();
  if (t0 == 0) *a.step = step0 + a.n_epochs;
}

// ReplayBuffer.add for every env (reference contain.py:15-17, called from value.py:114): phase 0, before env.step, stores the
// boards as the transitions' `state`; phase 1, after it, stores the boards as `successor` and the action / reward /
// terminal flag from the step records. One launch per phase instead of seven tensor copies per lockstep step.
__global__ __launch_bounds__(WG) void replay_store_kernel(const int8_t *__restrict__ boards, int pitch, int nc, int64_t n,
                                                          const uint32_t *__restrict__ rec, const uint8_t *__restrict__ actions,
                                                          int phase, int cheat, int64_t head, const long long *__restrict__ head_dev,
                                                          int8_t *__restrict__ states, int8_t *__restrict__ successors,
                                                          uint8_t *__restrict__ r_actions, int8_t *__restrict__ r_rewards,
                                                          uint8_t *__restrict__ r_terminals) {
  const int64_t slice = head_dev ? (int64_t)*head_dev : head;
  int8_t *dst = (phase == 0 ? states : successors) + slice * n * nc;
  const int64_t gtid = (int64_t)blockIdx.x * WG + threadIdx.x, gsz = (int64_t)gridDim.x * WG;
  if (pitch == nc && ((n * nc) & 3) == 0) {  // rows back to back: copy dwords
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(boards);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(dst);
    for (int64_t i = gtid; i < n * nc / 4; i += gsz) d32[i] = s32[i];
  } else {
    for (int64_t i = gtid; i < n * nc; i += gsz) dst[i] = boards[(i / nc) * pitch + i % nc];
  }
  if (phase == 1) {
    for (int64_t env = gtid; env < n; env += gsz) {
      const uint32_t r = rec[env];  // reward | hidden << 8 | done << 16 | actual action << 24
      // (& 3: an executed "stay", action 4 under a non-default SGK_INTERRUPT_FORCED_ACTION, has no Q column; it is stored as UP,
      // the default reading of that switch -- same trajectory in the level's corridor)
      r_actions[slice * n + env] = cheat ? (uint8_t)((r >> 24) & 3u) : actions[env];
      r_rewards[slice * n + env] = cheat ? (int8_t)(r >> 8) : (int8_t)r;
      r_terminals[slice * n + env] = (uint8_t)((r >> 16) & 1u);
    }
  }
}

hipError_t launch_replay_store(const Shard &sh, int phase, const uint8_t *actions, int cheat, int64_t head, const long long *head_dev,
                               int8_t *states, int8_t *successors, uint8_t *r_actions, int8_t *r_rewards, uint8_t *r_terminals,
                               hipStream_t st) {
  (void)hipGetLastError();
  int grid = grid_for((sh.n * sh.n_cells / 4 + WG - 1) / WG, sh.max_grid);
  replay_store_kernel<<<dim3(grid), dim3(WG), 0, st>>>(sh.boards, sh.pitch, sh.n_cells, sh.n, sh.rec, actions, phase, cheat, head,
                                                      head_dev, states, successors, r_actions, r_rewards, r_terminals);
  return hipGetLastError();
}

size_t dqn_sgd_lds_bytes(int n_cells, int n_hidden) {
  const size_t kp = (size_t)((n_cells + 3) & ~3), h = (size_t)n_hidden;
  return sizeof(float) * (4 * LB * h + h * (size_t)weight_stride((int)h) + 8 * h + 4 * h + 8 + 2 * LB * 4 + LB + 32 + LB + 3 * LB) + 2 * LB * kp + 64;
}

// the learner's parameters (ParamMap<n_cells, n_hidden>::P for the shapes with a kernel)
constexpr size_t dqn_param_count(int n_cells, int n_hidden) {
  return (size_t)n_hidden * n_cells + n_hidden + (size_t)n_hidden * n_hidden + n_hidden + 4 * (size_t)n_hidden + 4;
}
static_assert(dqn_param_count(36, 100) == ParamMap<36, 100>::P && dqn_param_count(63, 64) == ParamMap<63, 64>::P, "one parameter count");

// the handle's scratch block: AdamHeader + the flat gradient (two-launch Adam)
size_t dqn_sgd_scratch_bytes(int n_cells, int n_hidden) {
  return (sizeof(AdamHeader) + sizeof(float) * dqn_param_count(n_cells, n_hidden) + 255) & ~(size_t)255;
}

// sgk_dqn_sgd_step_members' workspace (the caller's): one AdamHeader + flat gradient per member, at a 16-byte aligned stride
size_t dqn_members_scratch_stride(int n_cells, int n_hidden) {
  return (sizeof(AdamHeader) + sizeof(float) * dqn_param_count(n_cells, n_hidden) + 15) & ~(size_t)15;
}

bool mlp_cells_have_kernel(int n_cells) { return mlp_cells_listed(n_cells); }

// the SGD kernel of one shape (the 160 KB dynamic-LDS opt-in is made on its first launch per device)
template <int K0, int H, bool MEMBERS, bool HYPER = false>
static hipError_t launch_sgd(const LearnArgs &a, int n_members, size_t lds, int device, hipStream_t st) {
  hipError_t ae = allow_dynamic_lds<dqn_sgd_kernel<K0, H, MEMBERS, HYPER>>(device, 160 * 1024);
  if (ae != hipSuccess) return ae;
  dqn_sgd_kernel<K0, H, MEMBERS, HYPER><<<dim3(n_members), dim3(LWG), lds, st>>>(a);
  return hipSuccess;
}

// one shape's launches: the SGD kernel and, with `adam`, dqn_adam_kernel behind it (the two-launch form without a fused reset)
template <int K0, int H>
static hipError_t launch_sgd_adam(const LearnArgs &a, int n_members, bool adam, size_t lds, int device, hipStream_t st) {
  hipError_t se = a.member_hyper                   ? launch_sgd<K0, H, true, true>(a, n_members, lds, device, st)
                  : (n_members > 1 || a.member_keys) ? launch_sgd<K0, H, true>(a, n_members, lds, device, st)
                                                   : launch_sgd<K0, H, false>(a, 1, lds, device, st);
  if (se != hipSuccess) return se;
  if (adam) {
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return le;
    const dim3 ag(n_members * ((ParamMap<K0, H>::P + 255) / 256));
    if (n_members > 1) dqn_adam_kernel<K0, H, true><<<ag, dim3(256), 0, st>>>(a);
    else dqn_adam_kernel<K0, H, false><<<ag, dim3(256), 0, st>>>(a);
  }
  return hipSuccess;
}

hipError_t launch_dqn_sgd(const Shard &sh, const DqnLearner &L, hipStream_t st) {
  (void)hipGetLastError();
  if (L.n_hidden > 128 || L.n_hidden < 4 || (L.n_hidden & 3) || L.batch < 1 || L.batch > LB || sh.n_cells > 64) return hipErrorInvalidValue;
  if ((L.n_hidden / 4) * (L.n_hidden / 4) + L.n_hidden > LWG) return hipErrorInvalidValue;  // tile lanes + bias lanes
  const size_t lds = dqn_sgd_lds_bytes(sh.n_cells, L.n_hidden);
  if (lds > 160u * 1024u) return hipErrorInvalidValue;
  const int n_members = L.n_members;
  if (n_members < 1 || sh.n % n_members != 0) return hipErrorInvalidValue;
  // members: the two-launch form on the caller's workspace only (no fused reset)
  if (n_members > 1 && (!L.scratch || L.reset_store)) return hipErrorInvalidValue;
  if ((int64_t)n_members * L.n_hidden * std::max(L.n_hidden, sh.n_cells) > (int64_t)UINT32_MAX) return hipErrorInvalidValue;  // MemberOffsets
  LearnArgs a;
  a.member_envs = sh.n / n_members; a.member_total = (int64_t)L.slices_filled * a.member_envs;
  a.member_keys = L.member_keys; a.scratch_stride = (int64_t)(L.scratch_stride / sizeof(float));
  a.member_hyper = L.member_hyper;
  if (a.member_hyper && (!L.scratch || L.reset_store)) return hipErrorInvalidValue;  // (the members' two-launch form only)
  a.states = L.states; a.successors = L.successors; a.actions = L.actions; a.rewards = L.rewards; a.terminals = L.terminals;
  a.n_envs = sh.n; a.total = (int64_t)L.slices_filled * sh.n; a.n_cells = sh.n_cells;
  a.w1 = L.w1; a.b1 = L.b1; a.w2 = L.w2; a.b2 = L.b2; a.w3 = L.w3; a.b3 = L.b3;
  a.w1t = L.w1t; a.w2t = L.w2t; a.w3t = L.w3t;
  for (int i = 0; i < 6; ++i) { a.m[i] = L.m[i]; a.v[i] = L.v[i]; a.vmax[i] = L.vmax[i]; }
  a.tw1t = L.tw1t; a.tb1 = L.tb1; a.tw2t = L.tw2t; a.tb2 = L.tb2; a.tw3 = L.tw3; a.tb3 = L.tb3;
  a.step = L.step; a.loss_out = L.loss_out; a.n_hidden = L.n_hidden; a.batch = L.batch;
  a.loss_mode = L.loss_mode; a.rows = L.rows; a.rows_out = L.rows_out;
  a.adam_scratch = reinterpret_cast<float *>(L.scratch);
  a.reward_scale = sh.rules_host.reward_scale;
  a.seed = sh.seed;
  a.lr = (float)L.lr; a.beta1 = (float)L.beta1; a.beta2 = (float)L.beta2; a.eps = (float)L.eps; a.discount = (float)L.discount;
  a.max_norm = (float)L.max_grad_norm;
  const bool adam = a.adam_scratch && !L.reset_store;
  hipError_t se = hipErrorInvalidValue;  // (what a hidden width without an instantiation leaves)
  SGK_DISPATCH_CELLS(sh.n_cells, {  // the shapes with an instantiation: the levels' board sizes x the learners' hidden widths
    se = sizes_dispatch(MlpLearnWidths{}, L.n_hidden, [&](auto width) {
      return launch_sgd_adam<K0, decltype(width)::value>(a, n_members, adam, lds, sh.device, st);
    });
  });
  if (se != hipSuccess) return se;
  if (L.reset_store) {  // Adam + reset_done + the next transitions' states in ONE launch behind the SGD kernel
    if (!a.adam_scratch) return hipErrorInvalidValue;  // (the two-launch form only: the gradient must leave the SGD kernel)
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return le;
    ResetStoreArgs r;
    r.rules = sh.rules_dev; r.state = sh.state; r.boards = sh.boards; r.n_resets = sh.n_resets; r.aux = sh.aux;
    r.n = sh.n; r.seed = sh.seed; r.env_base = sh.env_base;
    r.mode_flags = 1 | ((L.rs_flags & SGK_F_NO_BOARDS) ? 4 : 0);
    r.st = make_store(sh, L.rs_states_ring, nullptr, nullptr, nullptr, L.rs_slice, L.rs_slice_dev, L.rs_ring, 0);
    const int reset_blocks = grid_for((sh.n + WG - 1) / WG, sh.max_grid);
    SGK_DISPATCH_ENV_LAYOUT(sh.env_id, sh.layout, {
      if (Geom<E>::NC != sh.n_cells) return hipErrorInvalidValue;
      (void)sizes_dispatch(MlpLearnWidths{}, a.n_hidden, [&](auto width) {  // (a listed width: the SGD launch above took it)
        constexpr int HV = decltype(width)::value;
        const int adam_blocks = (ParamMap<Geom<E>::NC, HV>::P + 255) / 256;
        dqn_adam_reset_kernel<HV, E, L><<<dim3(adam_blocks + reset_blocks), dim3(256), 0, st>>>(a, adam_blocks, r);
        return hipSuccess;
      });
    });
  }
  return hipGetLastError();
}

#ifdef SGK_LEARN_TIMELINE
extern "C" __attribute__((visibility("default"))) int sgk_debug_learn_stamps(unsigned long long *out32) {
  (void)hipDeviceSynchronize();
  return (int)hipMemcpyFromSymbol(out32, HIP_SYMBOL(learn_stamps), sizeof(unsigned long long) * 32);
}
#endif

size_t ppo_epochs_lds_bytes(int n_cells, int n_hidden) { return ppo_lds_bytes((n_cells + 3) & ~3, n_hidden); }

template <int K0, int H, bool HYPER>
static hipError_t launch_ppo_kernel(const PpoArgs &a, int n_members, size_t lds, int device, hipStream_t st) {
  hipError_t ae = allow_dynamic_lds<ppo_epochs_kernel<K0, H, HYPER>>(device, 160 * 1024);
  if (ae != hipSuccess) return ae;
  ppo_epochs_kernel<K0, H, HYPER><<<dim3(n_members), dim3(LWG), lds, st>>>(a);
  return hipSuccess;
}

template <int K0, int H>
static hipError_t launch_ppo(const PpoArgs &a, int n_members, size_t lds, int device, hipStream_t st) {
  return a.member_hyper ? launch_ppo_kernel<K0, H, true>(a, n_members, lds, device, st)
                        : launch_ppo_kernel<K0, H, false>(a, n_members, lds, device, st);
}

hipError_t launch_ppo_epochs(const Shard &sh, const PpoLearner &P, hipStream_t st, int n_members, const uint64_t *member_keys,
                             const PpoMemberHyper *member_hyper) {
  (void)hipGetLastError();
  if (P.batch < 2 || P.batch > LB || P.n_epochs < 1 || P.horizon < 1 || P.n_trajectories < 1 || P.n_trajectories >= (1ll << 31))
    return hipErrorInvalidValue;
  if (n_members < 1 || P.n_trajectories % n_members != 0) return hipErrorInvalidValue;
  const size_t lds = ppo_epochs_lds_bytes(sh.n_cells, P.n_hidden);
  if (lds > 160u * 1024u) return hipErrorInvalidValue;
  PpoArgs a;
  a.states = P.states; a.actions = P.actions; a.returns = P.returns; a.lengths = P.lengths;
  a.T = P.horizon; a.N = P.n_trajectories; a.E = P.n_trajectories / n_members;
  a.member_keys = member_keys;
  a.member_hyper = member_hyper;
  a.w1 = P.w1; a.b1 = P.b1; a.w2 = P.w2; a.b2 = P.b2; a.wa = P.wa; a.ba = P.ba; a.wc = P.wc; a.bc = P.bc;
  a.w1t = P.w1t; a.w2t = P.w2t;
  for (int i = 0; i < 8; ++i) { a.m[i] = P.m[i]; a.v[i] = P.v[i]; }
  a.ow1t = P.ow1t; a.ob1 = P.ob1; a.ow2t = P.ow2t; a.ob2 = P.ob2; a.owa = P.owa; a.oba = P.oba;
  a.step = P.step; a.stats_out = P.stats_out; a.rows = P.rows; a.rows_out = P.rows_out;
  a.batch = P.batch; a.n_epochs = P.n_epochs; a.seed = sh.seed;
  a.lr = (float)P.lr; a.beta1 = (float)P.beta1; a.beta2 = (float)P.beta2; a.eps = (float)P.eps;
  a.clipping = (float)P.clipping; a.critic_coeff = (float)P.critic_coeff; a.entropy_bonus = (float)P.entropy_bonus;
  hipError_t le = hipErrorInvalidValue;  // (what a hidden width without an instantiation leaves)
  SGK_DISPATCH_CELLS(sh.n_cells, {
    le = sizes_dispatch(MlpLearnWidths{}, P.n_hidden, [&](auto width) {
      return launch_ppo<K0, decltype(width)::value>(a, n_members, lds, sh.device, st);
    });
  });
  if (le != hipSuccess) return le;
  return hipGetLastError();
}

}  // namespace sgk
