// sgk_ppo_cnn.hip -- PPOBaseAgent.learn (reference policy_base.py:64-131) for PPOCNNAgent (policy_cnn.py:17-81): all epochs of one
// learn() call on the device, three launches per epoch, no float atomics (sgk_ppo_cnn_epochs).
//
// The network (n_layers = 2, C channels, four actions):
//     trunk  = relu(conv3x3(relu(conv3x3(x, 1 -> C)), C -> C)) + conv1x1(x, 1 -> C)
//     actor  = linear(flatten(relu(conv3x3(trunk, C -> C))), C * cells -> 4)
//     critic = linear(flatten(relu(conv3x3(trunk, C -> C))), C * cells -> 1)
// Per epoch:
//   1. ppo_cnn_forward_kernel, one workgroup per minibatch sample: the row (the caller's, or sgk_ppo_epochs' stream-5 draw keyed by
//      (seed, Adam step, lengths): the same rows for the same rollout and step), the old policy's trunk + actor (read in place, no
//      gradient), then the current network. Writes the sample's logits, value, old logits, return and action, and its activations
//      (h1, relu(conv2), trunk, actor head, critic head) to the workspace.
//   2. ppo_cnn_backward_kernel, one workgroup per sample: every workgroup reads the batch's per-sample scalars and forms the
//      advantage statistics itself (policy_base.py:82-106: adv = r - V normalised by its mean and unbiased std and NOT detached, the
//      clipped surrogate, mse_loss, the Categorical entropy -- sgk_ppo_epochs' arithmetic), then back-propagates its own sample
//      through both heads, the residual split, conv2 and conv1 into its row of per-sample gradients workspace[b][P]. Workgroup 0
//      writes the epoch's stats.
//   3. ppo_cnn_adam_kernel, one lane per parameter: the per-sample gradients summed in sample order, Adam (torch defaults, no
//      amsgrad; bias corrections from the device step counter), the 14 tensors updated in place; the step advances once.
// Kernel boundaries instead of grid barriers: a dependent launch costs ~1.5 us, an in-launch grid barrier 4-10 us. The activations of
// a sample ((1 + 5 C) padded planes + the parameters: <= 50 KB) live in one workgroup's LDS; the convolutions are so small (~1e5
// multiply-adds per sample and epoch) that one lane per output with the weights in LDS is latency- and not FLOP-bound. Every sum
// runs in a fixed order: a call is deterministic and a captured replay equals the eager call bit for bit.
// sgk_ppo_cnn_epochs_members: the same three launches for n_members independent learners, the member on blockIdx.y (the MEMBERS
// instantiations below); every member works in its own slice of the workspace and reads only its own samples.
// sgk_ppo_cnn_epochs_trans: the same three launches for the two-board body (the CIN = 2 instantiations; 5 x 5 boards, the single
// learner): x is [previous board, board] -- two adjacent padded planes, the previous board from `prev_states` at the same flat row --
// conv1 is 2 -> C, the trunk's residual wb[co][0] x0 + wb[co][1] x1 + bb[co], the bottleneck's weight gradient 2 C entries. The row
// draw, the loss arithmetic, pc_adam and the step counter are the one-plane form's code. LDS at C = 8: forward 28.7 KB ((2 + 5 C)
// planes of 49 floats, 2 933 + 2 148 parameters), backward 27.9 KB ((2 + 10 C) planes, 2 933 parameters).
#include <algorithm>

#include "sgk_device.h"

extern "C" __device__ float __ockl_wfred_add_f32(float);

namespace sgk {

constexpr int PC_WG = 256;
constexpr int PC_SC = 16;  // floats of per-sample scalars in the workspace: logits [0..3], value [4], old logits [5..8], return [9],
                           // action [10] (int), row [12..13] (int64)

// CIN: the board planes the network reads. 1: the board; 2 (sgk_ppo_cnn_epochs_trans): [previous board, board], network.0.0.weight
// [C][2][3][3] and bottleneck.weight [C][2][1][1] -- every later offset, P and PO move by 10 C, nothing else changes shape.
template <int HH, int WW, int C, int CIN = 1>
struct PcGeom {
  static constexpr int NC = HH * WW, NF = C * NC, CI = CIN;
  static constexpr int PW = WW + 2, PL = (HH + 2) * PW;  // a plane with a zero border
  static constexpr int K2 = 9 * C * C;
  // the 14 parameter tensors in registration order, flattened back to back: network.0.0, network.1.0.0, bottleneck, actor_cnn.0,
  // actor_linear, critic_cnn.0, critic_linear (weight, bias each). The old policy's 10 actor-path tensors are the first 10.
  static constexpr int o_w1 = 0, o_b1 = o_w1 + 9 * C * CIN, o_w2 = o_b1 + C, o_b2 = o_w2 + K2, o_wb = o_b2 + C, o_bb = o_wb + C * CIN,
                       o_wa = o_bb + C, o_ba = o_wa + K2, o_la = o_ba + C, o_lab = o_la + 4 * NF, o_wv = o_lab + 4, o_bv = o_wv + K2,
                       o_lv = o_bv + C, o_lvb = o_lv + NF, P = o_lvb + 1, PO = o_wv;
  // LDS planes (X: CIN adjacent board planes, the current board last)
  static constexpr int X = 0, H1 = CIN, H2 = CIN + C, TR = CIN + 2 * C, AH = CIN + 3 * C, CH = CIN + 4 * C, ACT_PLANES = CIN + 5 * C;
  static constexpr int GA = ACT_PLANES, GC = GA + C, DT = GC + C, G2 = DT + C, G1 = G2 + C, BWD_PLANES = G1 + C;
  static constexpr int SAVE = 5 * C * NC;  // activations saved per sample: h1, relu(conv2), trunk, actor head, critic head
};

__host__ __device__ constexpr int pc_params(int H, int W, int C, int cin = 1) {
  return 9 * C * cin + C + 3 * (9 * C * C + C) + C * cin + C + 5 * C * H * W + 5;
}

// workspace: [0..63] header (the step counter at the epoch's start, int64) | per-sample scalars [64][PC_SC] | activations [batch][SAVE]
// | per-sample gradients [batch][P]
constexpr size_t PC_HDR = 64, PC_SCAL = 64 * PC_SC;

size_t ppo_cnn_workspace_bytes(int height, int width, int n_channels, int batch, int in_channels) {
  const size_t save = (size_t)5 * n_channels * height * width, p = (size_t)pc_params(height, width, n_channels, in_channels);
  return sizeof(float) * (PC_HDR + PC_SCAL + (size_t)batch * (save + p));
}

// a member's slice of sgk_ppo_cnn_epochs_members' workspace: the single learner's layout, padded so that every slice's int64 header
// and rows stay 8-byte aligned
size_t ppo_cnn_members_stride_bytes(int height, int width, int n_channels, int batch) {
  return (ppo_cnn_workspace_bytes(height, width, n_channels, batch) + 7) & ~(size_t)7;
}

template <class G>
__device__ __forceinline__ int pc_cell(int cell) {  // interior cell -> its offset inside a padded plane
  const int y = cell / (G::PW - 2), x = cell - y * (G::PW - 2);
  return (y + 1) * G::PW + x + 1;
}

struct PpoCnnArgs {
  const int8_t *states;
  const uint8_t *actions;
  const float *returns;
  const int32_t *lengths;
  int32_t T;
  int64_t N;
  float *p[14], *m[14], *v[14];
  const float *o[10];
  long long *step;
  float *stats_out;
  const long long *rows;
  long long *rows_out;
  float *ws;
  int32_t batch;
  uint64_t seed;
  float lr, beta1, beta2, eps, clipping, critic_coeff, entropy_bonus;
  // the member instantiation only (sgk_ppo_cnn_epochs_members): blockIdx.y = member m. Every tensor above but the rollout is stacked
  // [n_members][...] and the pointers address member 0; the workspace is n_members slices of ws_stride floats; member m draws from
  // the trajectories m * E .. (m + 1) * E - 1 with member_keys[m] (null: `seed`) and step[m]
  int64_t E;
  const uint64_t *member_keys;
  size_t ws_stride;
  int32_t n_epochs;
  // the HYPER instantiations only (sgk_ppo_cnn_epochs_members_hyper): [n_members], member m's lr / clipping / critic_coeff /
  // entropy_bonus instead of the four above
  const PpoMemberHyper *member_hyper;
};
// the two-plane kernels' argument (sgk_ppo_cnn_epochs_trans): the new pointer behind everything above. A type of its own, because
// `epoch` follows the struct in the forward and backward kernels' argument lists: a member appended to PpoCnnArgs itself would move
// that offset in every one-plane kernel.
struct PpoCnnTransArgs : PpoCnnArgs {
  const int8_t *prev_states;  // int8 [T][N][cells]: plane 0 of row t * N + n (plane 1 is `states`)
};
template <int CIN>
struct PcArgs { typedef PpoCnnArgs type; };
template <>
struct PcArgs<2> { typedef PpoCnnTransArgs type; };

// this workgroup's member (0 without the member axis) and what it owns
template <bool MEMBERS>
__device__ __forceinline__ size_t pc_member() { return MEMBERS ? (size_t)blockIdx.y : (size_t)0; }
template <bool MEMBERS>
__device__ __forceinline__ float *pc_ws(const PpoCnnArgs &a) { return MEMBERS ? a.ws + pc_member<MEMBERS>() * a.ws_stride : a.ws; }

template <class G>
__device__ __forceinline__ int pc_tensor_size(int k) {
  constexpr int off[15] = {G::o_w1, G::o_b1, G::o_w2, G::o_b2, G::o_wb, G::o_bb, G::o_wa, G::o_ba, G::o_la, G::o_lab, G::o_wv, G::o_bv,
                           G::o_lv, G::o_lvb, G::P};
  return off[k + 1] - off[k];
}

// the first n_tensors parameter tensors (member `member`'s slice of each), flattened, into LDS
template <class G>
__device__ __forceinline__ void pc_stage(float *dst, const float *const *src, int n_tensors, size_t member) {
  int base = 0;
  for (int k = 0; k < n_tensors; ++k) {
    const int n = pc_tensor_size<G>(k);
    const float *sk = src[k] + member * (size_t)n;
    for (int i = threadIdx.x; i < n; i += PC_WG) dst[base + i] = sk[i];
    base += n;
  }
}

// out[co] = act(b[co] + sum_{ci, ky, kx} w[co][ci][ky][kx] in[ci](y + ky - 1, x + kx - 1)), one lane per (co, cell).
// MODE 0: ReLU; MODE 1: ReLU, and the trunk plane trunk_out[co] = that + sum_k wb[co][k] * x_k + bb[co] over the G::CI board planes
// (summed from the last plane to the first) as well (out = relu(conv2) is kept)
template <class G, int CIN, int C, int MODE>
__device__ __forceinline__ void pc_conv(float *act, int in_plane, int out_plane, const float *w, const float *b, const float *wb = nullptr,
                                        const float *bb = nullptr, int trunk_plane = 0) {
  for (int i = threadIdx.x; i < C * G::NC; i += PC_WG) {
    const int co = i / G::NC, cell = i - co * G::NC;
    const int c0 = pc_cell<G>(cell) - G::PW - 1;  // the window's top-left corner
    const float *wr = w + co * 9 * CIN;
    float acc = b[co];
    for (int ci = 0; ci < CIN; ++ci) {
      const float *ip = act + (in_plane + ci) * G::PL + c0;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) acc = fmaf(wr[ci * 9 + ky * 3 + kx], ip[ky * G::PW + kx], acc);
    }
    const float r = fmaxf(acc, 0.0f);
    act[(out_plane + co) * G::PL + c0 + G::PW + 1] = r;
    if constexpr (MODE == 1 && G::CI == 2) {
      const float x0 = act[G::X * G::PL + c0 + G::PW + 1], x1 = act[(G::X + 1) * G::PL + c0 + G::PW + 1];
      act[(trunk_plane + co) * G::PL + c0 + G::PW + 1] = r + fmaf(wb[2 * co], x0, fmaf(wb[2 * co + 1], x1, bb[co]));
    } else if (MODE == 1) {
      act[(trunk_plane + co) * G::PL + c0 + G::PW + 1] = r + fmaf(wb[co], act[G::X * G::PL + c0 + G::PW + 1], bb[co]);
    }
  }
}

// NOUT linear outputs (bias + weights [NOUT][C * cells] . flatten(planes)) summed in a fixed order: lane partials, wave sums, then
// the four waves in order. Result in red[0 .. NOUT - 1] behind the trailing barrier.
template <class G, int NOUT>
__device__ __forceinline__ void pc_linear(const float *act, int plane, const float *w, const float *b, float *red) {
  float s[NOUT];
#pragma unroll
  for (int o = 0; o < NOUT; ++o) s[o] = 0.0f;
  for (int f = threadIdx.x; f < G::NF; f += PC_WG) {
    const int c = f / G::NC, cell = f - c * G::NC;
    const float h = act[(plane + c) * G::PL + pc_cell<G>(cell)];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) s[o] = fmaf(w[o * G::NF + f], h, s[o]);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
    const float ws = __ockl_wfred_add_f32(s[o]);
    if (lane == 0) red[8 + wave * 8 + o] = ws;
  }
  __syncthreads();
  if (threadIdx.x < NOUT) {
    float t = b[threadIdx.x];
    for (int w = 0; w < PC_WG / 64; ++w) t += red[8 + w * 8 + threadIdx.x];
    red[threadIdx.x] = t;
  }
  __syncthreads();
}

// the trunk of the network whose flat parameters are at `w`, on the board planes at X: h1, relu(conv2) and the trunk planes
template <class G, int C>
__device__ __forceinline__ void pc_trunk(float *act, const float *w) {
  pc_conv<G, G::CI, C, 0>(act, G::X, G::H1, w + G::o_w1, w + G::o_b1);
  __syncthreads();
  pc_conv<G, C, C, 1>(act, G::H1, G::H2, w + G::o_w2, w + G::o_b2, w + G::o_wb, w + G::o_bb, G::TR);
  __syncthreads();
}

// MEMBERS = false: sgk_ppo_cnn_epochs' kernels, grid (batch) resp. (ceil(P / 256)); MEMBERS = true: sgk_ppo_cnn_epochs_members', a
// member axis blockIdx.y on the same grids (with one member too). The arithmetic of a sample does not depend on the flag.
// CIN = 2 (sgk_ppo_cnn_epochs_trans; the single learner only): two board planes, the previous board from a.prev_states.
template <int HH, int WW, int C, bool MEMBERS, int CIN = 1>
__global__ __launch_bounds__(PC_WG) void ppo_cnn_forward_kernel(typename PcArgs<CIN>::type a, int epoch) {
  static_assert(CIN == 1 || !MEMBERS, "the two-plane form has no member axis");
  typedef PcGeom<HH, WW, C, CIN> G;
  __shared__ __attribute__((aligned(16))) float act[G::ACT_PLANES * G::PL];
  __shared__ __attribute__((aligned(16))) float wcur[G::P];
  __shared__ __attribute__((aligned(16))) float wold[G::PO];
  __shared__ float red[8 + 8 * (PC_WG / 64)];
  __shared__ long long row_s;
  const int b = blockIdx.x, t = threadIdx.x, B = a.batch;
  const size_t mem = pc_member<MEMBERS>();
  float *ws = pc_ws<MEMBERS>(a);
  float *sc = ws + PC_HDR + b * PC_SC;
  const long long step = a.step[mem];  // Adam steps done before this epoch: the key of the draws
  const long long slot = MEMBERS ? ((long long)mem * a.n_epochs + epoch) * B + b : (long long)epoch * B + b;  // in rows / rows_out
  const long long n0 = MEMBERS ? (long long)mem * a.E : 0, NE = MEMBERS ? a.E : a.N;  // this learner's trajectories: n0 .. n0 + NE - 1
  uint64_t seed = a.seed;
  if (MEMBERS && a.member_keys) seed = a.member_keys[mem];
  // ---- the row: the caller's, or sgk_ppo_epochs' draw (16 candidates per round, the first valid one in candidate order) ----
  if (t < 64) {
    const int lane = t;
    long long row;
    if (a.rows) {
      row = a.rows[slot];
      if (MEMBERS) {  // a row outside the rollout or of another member's trajectory: the member's first row (step 0, trajectory n0)
        const bool inside = row >= 0 && row < (long long)a.T * a.N;
        const long long nn = inside ? row % a.N : -1;
        if (nn < n0 || nn >= n0 + NE) row = n0;
      } else {
        row = row < 0 ? 0 : (row >= (long long)a.T * a.N ? (long long)a.T * a.N - 1 : row);  // a bad row must not leave the rollout
      }
    } else {
      int tt = 0, nn = (int)n0;
      for (int round = 0; round < 64; ++round) {
        bool ok = false;
        int t_c = 0, n_c = 0;
        if (lane < 16) {
          uint32_t x[4];
          philox4x32_10((uint32_t)(b * 16 + lane), (uint32_t)round, (uint32_t)step, 5u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
          n_c = (int)n0 + (int)__umul64hi(((unsigned long long)x[0] << 32) | x[1], (unsigned long long)NE);
          t_c = (int)__umulhi(x[2], (uint32_t)a.T);
          ok = t_c < a.lengths[n_c];
        }
        const unsigned long long mask = __ballot(ok) & 0xffffull;
        if (mask) {
          const int win = __ffsll((long long)mask) - 1;
          tt = __shfl(t_c, win, 64);
          nn = __shfl(n_c, win, 64);
          break;
        }
      }
      row = (long long)tt * a.N + nn;
    }
    if (lane == 0) {
      row_s = row;
      const long long tt = row / a.N, nn = row - tt * a.N;
      sc[9] = a.returns[nn * a.T + tt];
      reinterpret_cast<int *>(sc)[10] = (int)(a.actions[row] & 3);
      *reinterpret_cast<long long *>(sc + 12) = row;
      if (a.rows_out) a.rows_out[slot] = row;
      if (b == 0) *reinterpret_cast<long long *>(ws) = step;
    }
  }
  for (int i = t; i < G::ACT_PLANES * G::PL; i += PC_WG) act[i] = 0.0f;
  pc_stage<G>(wcur, a.p, 14, mem);
  pc_stage<G>(wold, a.o, 10, mem);
  __syncthreads();
  {  // the board: the last of the CIN planes at X; the previous board in front of it
    const int8_t *board = a.states + row_s * G::NC;
    for (int i = t; i < G::NC; i += PC_WG) act[(G::X + CIN - 1) * G::PL + pc_cell<G>(i)] = (float)board[i];
    if constexpr (CIN == 2) {
      const int8_t *prev = a.prev_states + row_s * G::NC;
      for (int i = t; i < G::NC; i += PC_WG) act[G::X * G::PL + pc_cell<G>(i)] = (float)prev[i];
    }
  }
  __syncthreads();
  // ---- the old policy: trunk + actor (no gradient) ----
  pc_trunk<G, C>(act, wold);
  pc_conv<G, C, C, 0>(act, G::TR, G::AH, wold + G::o_wa, wold + G::o_ba);
  __syncthreads();
  pc_linear<G, 4>(act, G::AH, wold + G::o_la, wold + G::o_lab, red);
  if (t < 4) sc[5 + t] = red[t];
  // ---- the current network: trunk, actor head, critic head ----
  pc_trunk<G, C>(act, wcur);
  pc_conv<G, C, C, 0>(act, G::TR, G::AH, wcur + G::o_wa, wcur + G::o_ba);
  pc_conv<G, C, C, 0>(act, G::TR, G::CH, wcur + G::o_wv, wcur + G::o_bv);
  __syncthreads();
  pc_linear<G, 4>(act, G::AH, wcur + G::o_la, wcur + G::o_lab, red);
  if (t < 4) sc[t] = red[t];
  pc_linear<G, 1>(act, G::CH, wcur + G::o_lv, wcur + G::o_lvb, red);
  if (t == 0) sc[4] = red[0];
  // ---- the activations the backward pass needs ----
  float *save = ws + PC_HDR + PC_SCAL + (size_t)b * G::SAVE;
  for (int i = t; i < G::SAVE; i += PC_WG) {
    const int pl = i / G::NC, cell = i - pl * G::NC;
    save[i] = act[(G::H1 + pl) * G::PL + pc_cell<G>(cell)];
  }
}

// g_out planes (interior) -> the gradient of the 3 x 3 weights and biases: dw[co][ci][ky][kx] = sum_cells g[co](y, x) in[ci](y + ky - 1,
// x + kx - 1), db[co] = sum_cells g[co]; one lane per weight, cells in order
template <class G, int CIN, int C>
__device__ __forceinline__ void pc_wgrad(const float *act, int g_plane, int in_plane, float *dw, float *db) {
  for (int i = threadIdx.x; i < C * CIN * 9 + C; i += PC_WG) {
    float acc = 0.0f;
    if (i < C * CIN * 9) {
      const int co = i / (CIN * 9), r = i - co * CIN * 9, ci = r / 9, k = r - ci * 9, ky = k / 3, kx = k - ky * 3;
      const float *gp = act + (g_plane + co) * G::PL, *ip = act + (in_plane + ci) * G::PL + (ky - 1) * G::PW + (kx - 1);
      for (int cell = 0; cell < G::NC; ++cell) {
        const int o = pc_cell<G>(cell);
        acc = fmaf(gp[o], ip[o], acc);
      }
      dw[i] = acc;
    } else {
      const int co = i - C * CIN * 9;
      const float *gp = act + (g_plane + co) * G::PL;
      for (int cell = 0; cell < G::NC; ++cell) acc += gp[pc_cell<G>(cell)];
      db[co] = acc;
    }
  }
}

// the input gradient of a 3 x 3 convolution (C -> C): d_in[ci](y, x) = sum_{co, ky, kx} w[co][ci][ky][kx] g[co](y + 1 - ky, x + 1 - kx)
// (zero border), one lane per (ci, cell); returned per lane through `f(ci, offset, value)`
template <class G, int C, class F>
__device__ __forceinline__ void pc_input_grad(const float *act, int g_plane, const float *w, F &&f) {
  for (int i = threadIdx.x; i < C * G::NC; i += PC_WG) {
    const int ci = i / G::NC, cell = i - ci * G::NC;
    const int o = pc_cell<G>(cell);
    float acc = 0.0f;
    for (int co = 0; co < C; ++co) {
      const float *gp = act + (g_plane + co) * G::PL + o + G::PW + 1;
      const float *wr = w + (co * C + ci) * 9;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) acc = fmaf(wr[ky * 3 + kx], gp[-ky * G::PW - kx], acc);
    }
    f(ci, o, acc);
  }
}

// HYPER = true (with MEMBERS; sgk_ppo_cnn_epochs_members_hyper): the member coordinate loads its element of a.member_hyper once at
// entry -- a wave-uniform load -- and converts each field with the host's (float) cast. The forward kernel reads none of the four.
template <int HH, int WW, int C, bool MEMBERS, bool HYPER = false, int CIN = 1>
__global__ __launch_bounds__(PC_WG) void ppo_cnn_backward_kernel(typename PcArgs<CIN>::type a, int epoch) {
  static_assert(MEMBERS || !HYPER, "per-member hyper-parameters come with the member axis");
  static_assert(CIN == 1 || !MEMBERS, "the two-plane form has no member axis");
  typedef PcGeom<HH, WW, C, CIN> G;
  __shared__ __attribute__((aligned(16))) float act[G::BWD_PLANES * G::PL];
  __shared__ __attribute__((aligned(16))) float w[G::P];
  __shared__ float dout[8];
  const int b = blockIdx.x, t = threadIdx.x, B = a.batch;
  const size_t mem = pc_member<MEMBERS>();
  if constexpr (HYPER) {
    const PpoMemberHyper hp = a.member_hyper[mem];
    a.clipping = (float)hp.clipping; a.critic_coeff = (float)hp.critic_coeff; a.entropy_bonus = (float)hp.entropy_bonus;
  }
  float *ws = pc_ws<MEMBERS>(a);
  const float *scal = ws + PC_HDR;  // this member's own samples
  for (int i = t; i < G::BWD_PLANES * G::PL; i += PC_WG) act[i] = 0.0f;
  pc_stage<G>(w, a.p, 14, mem);
  __syncthreads();
  {
    const long long row = *reinterpret_cast<const long long *>(scal + b * PC_SC + 12);
    const int8_t *board = a.states + row * G::NC;
    for (int i = t; i < G::NC; i += PC_WG) act[(G::X + CIN - 1) * G::PL + pc_cell<G>(i)] = (float)board[i];
    if constexpr (CIN == 2) {
      const int8_t *prev = a.prev_states + row * G::NC;
      for (int i = t; i < G::NC; i += PC_WG) act[G::X * G::PL + pc_cell<G>(i)] = (float)prev[i];
    }
    const float *save = ws + PC_HDR + PC_SCAL + (size_t)b * G::SAVE;
    for (int i = t; i < G::SAVE; i += PC_WG) {
      const int pl = i / G::NC, cell = i - pl * G::NC;
      act[(G::H1 + pl) * G::PL + pc_cell<G>(cell)] = save[i];
    }
  }
  // ---- losses and dL/d(logits, value) of this workgroup's sample: the batch's samples are the lanes of wave 0 (sgk_ppo_epochs'
  // arithmetic, statistics by wave reductions) ----
  if (t < 64) {
    const int lane = t;
    const bool live = lane < B;
    const float *s = scal + (live ? lane : 0) * PC_SC;
    const float invB = 1.0f / (float)B;
    float l[4], lo[4], p[4], logp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { l[k] = s[k]; lo[k] = s[5 + k]; }
    const float v = s[4], r = s[9];
    const int ac = reinterpret_cast<const int *>(s)[10];
    const float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3])), mxo = fmaxf(fmaxf(lo[0], lo[1]), fmaxf(lo[2], lo[3]));
    const float lse = mx + logf(expf(l[0] - mx) + expf(l[1] - mx) + expf(l[2] - mx) + expf(l[3] - mx));
    const float lseo = mxo + logf(expf(lo[0] - mxo) + expf(lo[1] - mxo) + expf(lo[2] - mxo) + expf(lo[3] - mxo));
    float ent = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { logp[k] = l[k] - lse; p[k] = expf(logp[k]); ent -= p[k] * logp[k]; }
    const float logp_a = ac == 0 ? logp[0] : ac == 1 ? logp[1] : ac == 2 ? logp[2] : logp[3];
    const float lo_a = (ac == 0 ? lo[0] : ac == 1 ? lo[1] : ac == 2 ? lo[2] : lo[3]) - lseo;
    const float ratio = expf(logp_a - lo_a);
    const float adv = live ? r - v : 0.0f;
    const float mu = __ockl_wfred_add_f32(adv) * invB;
    const float dev = live ? adv - mu : 0.0f;
    const float sigma = sqrtf(__ockl_wfred_add_f32(dev * dev) / (float)(B - 1));
    const float advn = dev / sigma;
    const float lo_c = 1.0f - a.clipping, hi_c = 1.0f + a.clipping;
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
    const float dv = live ? a.critic_coeff * 2.0f * (v - r) * invB - g_adv : 0.0f;
    if (lane == b) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float onehot = k == ac ? 1.0f : 0.0f;
        dout[k] = g_logp * (onehot - p[k]) + a.entropy_bonus * invB * p[k] * (logp[k] + ent);
      }
      dout[4] = dv;
    }
    if (b == 0 && a.stats_out) {
      const float pl = -__ockl_wfred_add_f32(live ? fminf(s1, s2) : 0.0f) * invB;
      const float vl = __ockl_wfred_add_f32(live ? (v - r) * (v - r) : 0.0f) * invB;
      const float en = __ockl_wfred_add_f32(live ? ent : 0.0f) * invB;
      float *so = a.stats_out + (MEMBERS ? (mem * a.n_epochs + epoch) * 3 : (size_t)epoch * 3);
      if (lane == 0) { so[0] = pl; so[1] = vl; so[2] = en; }
    }
  }
  __syncthreads();
  float *g = ws + PC_HDR + PC_SCAL + (size_t)B * G::SAVE + (size_t)b * G::P;  // this sample's gradient row
  // ---- the linear heads: weight / bias gradients, and the heads' pre-activation gradients (ReLU') into GA / GC ----
  for (int f = t; f < G::NF; f += PC_WG) {
    const int c = f / G::NC, cell = f - c * G::NC, o = pc_cell<G>(cell);
    const float ha = act[(G::AH + c) * G::PL + o], hc = act[(G::CH + c) * G::PL + o];
    float da = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      g[G::o_la + k * G::NF + f] = dout[k] * ha;
      da = fmaf(dout[k], w[G::o_la + k * G::NF + f], da);
    }
    g[G::o_lv + f] = dout[4] * hc;
    act[(G::GA + c) * G::PL + o] = ha > 0.0f ? da : 0.0f;
    act[(G::GC + c) * G::PL + o] = hc > 0.0f ? dout[4] * w[G::o_lv + f] : 0.0f;
  }
  if (t < 4) g[G::o_lab + t] = dout[t];
  if (t == 4) g[G::o_lvb] = dout[4];
  __syncthreads();
  // ---- the head convolutions' weights, and d trunk = both heads' input gradients ----
  pc_wgrad<G, C, C>(act, G::GA, G::TR, g + G::o_wa, g + G::o_ba);
  pc_wgrad<G, C, C>(act, G::GC, G::TR, g + G::o_wv, g + G::o_bv);
  pc_input_grad<G, C>(act, G::GA, w + G::o_wa, [&](int ci, int o, float v) { act[(G::DT + ci) * G::PL + o] = v; });
  __syncthreads();
  pc_input_grad<G, C>(act, G::GC, w + G::o_wv, [&](int ci, int o, float v) {
    const float d = act[(G::DT + ci) * G::PL + o] + v;
    act[(G::DT + ci) * G::PL + o] = d;
    act[(G::G2 + ci) * G::PL + o] = act[(G::H2 + ci) * G::PL + o] > 0.0f ? d : 0.0f;  // the residual split: relu(conv2)'s share
  });
  __syncthreads();
  // ---- the bottleneck (1 x 1 on the board planes: entry [c][k] = d_trunk[c] . x_k, cells in order) and conv2 ----
  if constexpr (CIN == 2) {
    if (t < 3 * C) {
      const int c = t < 2 * C ? t >> 1 : t - 2 * C;
      const float *dp = act + (G::DT + c) * G::PL, *xp = act + (G::X + (t & 1)) * G::PL;
      float acc = 0.0f;
      for (int cell = 0; cell < G::NC; ++cell) {
        const int o = pc_cell<G>(cell);
        acc = t < 2 * C ? fmaf(dp[o], xp[o], acc) : acc + dp[o];
      }
      g[t < 2 * C ? G::o_wb + t : G::o_bb + c] = acc;
    }
  } else if (t < 2 * C) {
    const int c = t % C;
    const float *dp = act + (G::DT + c) * G::PL;
    float acc = 0.0f;
    for (int cell = 0; cell < G::NC; ++cell) {
      const int o = pc_cell<G>(cell);
      acc = t < C ? fmaf(dp[o], act[G::X * G::PL + o], acc) : acc + dp[o];
    }
    g[(t < C ? G::o_wb : G::o_bb) + c] = acc;
  }
  pc_wgrad<G, C, C>(act, G::G2, G::H1, g + G::o_w2, g + G::o_b2);
  pc_input_grad<G, C>(act, G::G2, w + G::o_w2, [&](int ci, int o, float v) {
    act[(G::G1 + ci) * G::PL + o] = act[(G::H1 + ci) * G::PL + o] > 0.0f ? v : 0.0f;
  });
  __syncthreads();
  // ---- conv1 (no input gradient) ----
  pc_wgrad<G, G::CI, C>(act, G::G1, G::X, g + G::o_w1, g + G::o_b1);
}

__device__ __forceinline__ float pc_adam(float p, float &m, float &v, float g, float lr_bc1, float inv_bc2_sqrt, float beta1, float beta2,
                                         float eps) {
  m = m + (1.0f - beta1) * (g - m);
  v = beta2 * v + (1.0f - beta2) * g * g;
  return p - lr_bc1 * (m * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) * inv_bc2_sqrt + eps));  // (sgk_ppo_epochs' adam_plain)
}

template <int HH, int WW, int C, bool MEMBERS, bool HYPER = false, int CIN = 1>
__global__ __launch_bounds__(PC_WG) void ppo_cnn_adam_kernel(typename PcArgs<CIN>::type a) {
  static_assert(MEMBERS || !HYPER, "per-member hyper-parameters come with the member axis");
  typedef PcGeom<HH, WW, C, CIN> G;
  const int e = blockIdx.x * PC_WG + threadIdx.x;
  const size_t mem = pc_member<MEMBERS>();
  if constexpr (HYPER) a.lr = (float)a.member_hyper[mem].lr;
  const float *ws = pc_ws<MEMBERS>(a);
  const long long step = *reinterpret_cast<const long long *>(ws);  // (the forward launch's copy: the step counter is written below)
  if (e < G::P) {
    const float *gr = ws + PC_HDR + PC_SCAL + (size_t)a.batch * G::SAVE + e;
    float gs = 0.0f;
    for (int b = 0; b < a.batch; ++b) gs += gr[(size_t)b * G::P];
    constexpr int off[14] = {G::o_w1, G::o_b1, G::o_w2, G::o_b2, G::o_wb, G::o_bb, G::o_wa, G::o_ba, G::o_la, G::o_lab, G::o_wv, G::o_bv,
                             G::o_lv, G::o_lvb};
    int k = 0;
#pragma unroll
    for (int j = 1; j < 14; ++j) k += e >= off[j] ? 1 : 0;
    const int le = e - off[k];
    const size_t mo = MEMBERS ? mem * (size_t)pc_tensor_size<G>(k) : (size_t)0;  // this member's slice of tensor k
    float *pk = a.p[k] + mo, *mk = a.m[k] + mo, *vk = a.v[k] + mo;
    const float lr_bc1 = a.lr / (float)(1.0 - pow((double)a.beta1, (double)(step + 1)));
    const float inv_bc2_sqrt = 1.0f / sqrtf((float)(1.0 - pow((double)a.beta2, (double)(step + 1))));
    float m = mk[le], v = vk[le];
    pk[le] = pc_adam(pk[le], m, v, gs, lr_bc1, inv_bc2_sqrt, a.beta1, a.beta2, a.eps);
    mk[le] = m;
    vk[le] = v;
  }
  if (e == 0) a.step[mem] = step + 1;
}

// the shapes of the acting kernels, through their lists (sgk_shapes.h)
bool ppo_cnn_shape_supported(int height, int width, int n_channels) {
  return cq_board_listed(CqOneBoardShapes{}, height, width) && sizes_listed(CqChannels{}, n_channels);
}

template <int HH, int WW, int C, bool MEMBERS, bool HYPER = false, int CIN = 1>
static hipError_t launch_ppo_cnn_shape(const typename PcArgs<CIN>::type &a, int n_epochs, int n_members, hipStream_t st) {
  typedef PcGeom<HH, WW, C, CIN> G;
  static_assert(G::P == pc_params(HH, WW, C, CIN), "parameter map");
  static_assert(G::P == PcGeom<HH, WW, C>::P + 10 * C * (CIN - 1) && G::PO == PcGeom<HH, WW, C>::PO + 10 * C * (CIN - 1), "the second plane's share");
  const unsigned ny = MEMBERS ? (unsigned)n_members : 1u;
  for (int epoch = 0; epoch < n_epochs; ++epoch) {
    ppo_cnn_forward_kernel<HH, WW, C, MEMBERS, CIN><<<dim3(a.batch, ny), dim3(PC_WG), 0, st>>>(a, epoch);
    ppo_cnn_backward_kernel<HH, WW, C, MEMBERS, HYPER, CIN><<<dim3(a.batch, ny), dim3(PC_WG), 0, st>>>(a, epoch);
    ppo_cnn_adam_kernel<HH, WW, C, MEMBERS, HYPER, CIN><<<dim3((G::P + PC_WG - 1) / PC_WG, ny), dim3(PC_WG), 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// what both entry points refuse
static bool pc_learner_ok(const PpoCnnLearner &P) {
  return P.batch >= 2 && P.batch <= 64 && P.n_epochs >= 1 && P.horizon >= 1 && P.n_trajectories >= 1 && P.n_trajectories < (1ll << 31) &&
         P.workspace;
}

// the kernels' argument from the learner (everything but what the member and two-plane forms add)
static void pc_fill_args(PpoCnnArgs &a, const Shard &sh, const PpoCnnLearner &P) {
  a.states = P.states; a.actions = P.actions; a.returns = P.returns; a.lengths = P.lengths;
  a.T = P.horizon; a.N = P.n_trajectories;
  for (int i = 0; i < 14; ++i) { a.p[i] = P.p[i]; a.m[i] = P.m[i]; a.v[i] = P.v[i]; }
  for (int i = 0; i < 10; ++i) a.o[i] = P.o[i];
  a.step = P.step; a.stats_out = P.stats_out; a.rows = P.rows; a.rows_out = P.rows_out;
  a.ws = reinterpret_cast<float *>(P.workspace);
  a.batch = P.batch; a.seed = sh.seed;
  a.lr = (float)P.lr; a.beta1 = (float)P.beta1; a.beta2 = (float)P.beta2; a.eps = (float)P.eps;
  a.clipping = (float)P.clipping; a.critic_coeff = (float)P.critic_coeff; a.entropy_bonus = (float)P.entropy_bonus;
  a.E = P.n_trajectories;
  a.member_keys = nullptr;
  a.ws_stride = 0;
  a.n_epochs = P.n_epochs;
  a.member_hyper = nullptr;
}

hipError_t launch_ppo_cnn_epochs(const Shard &sh, const PpoCnnLearner &P, hipStream_t st, int n_members, const uint64_t *member_keys,
                                 const PpoMemberHyper *member_hyper) {
  (void)hipGetLastError();
  const int H = sh.rules_host.height, W = sh.rules_host.width, C = P.n_channels;
  if (!ppo_cnn_shape_supported(H, W, C) || !pc_learner_ok(P)) return hipErrorInvalidValue;
  if (n_members < 0 || n_members > 65535 || (n_members > 0 && P.n_trajectories % n_members != 0)) return hipErrorInvalidValue;  // (gridDim.y)
  if (member_hyper && n_members < 1) return hipErrorInvalidValue;
  PpoCnnArgs a;
  pc_fill_args(a, sh, P);
  a.E = n_members > 0 ? P.n_trajectories / n_members : P.n_trajectories;
  a.member_keys = member_keys;
  a.ws_stride = ppo_cnn_members_stride_bytes(H, W, C, P.batch) / sizeof(float);
  a.n_epochs = P.n_epochs;
  a.member_hyper = member_hyper;
  return cq_dispatch(CqOneBoardShapes{}, H, W, C, [&](auto board, auto channels) {
    constexpr int HV = decltype(board)::H, WV = decltype(board)::W, CV = decltype(channels)::value;
    if (member_hyper) return launch_ppo_cnn_shape<HV, WV, CV, true, true>(a, P.n_epochs, n_members, st);
    if (n_members > 0) return launch_ppo_cnn_shape<HV, WV, CV, true>(a, P.n_epochs, n_members, st);
    return launch_ppo_cnn_shape<HV, WV, CV, false>(a, P.n_epochs, 1, st);
  });
}

bool ppo_cnn_trans_shape_supported(int height, int width, int n_channels) {  // the shapes sgk_convq_*_trans act on
  return cq_board_listed(CqTwoBoardShapes{}, height, width) && sizes_listed(CqChannels{}, n_channels);
}

hipError_t launch_ppo_cnn_epochs_trans(const Shard &sh, const PpoCnnLearner &P, const int8_t *prev_states, hipStream_t st) {
  (void)hipGetLastError();
  const int C = P.n_channels;
  if (!ppo_cnn_trans_shape_supported(sh.rules_host.height, sh.rules_host.width, C) || !pc_learner_ok(P) || !prev_states)
    return hipErrorInvalidValue;
  PpoCnnTransArgs a;
  pc_fill_args(a, sh, P);
  a.prev_states = prev_states;
  return cq_dispatch(CqTwoBoardShapes{}, sh.rules_host.height, sh.rules_host.width, C, [&](auto board, auto channels) {
    return launch_ppo_cnn_shape<decltype(board)::H, decltype(board)::W, decltype(channels)::value, false, false, 2>(a, P.n_epochs, 1, st);
  });
}

}  // namespace sgk
