// Evaluation tail of main_dca.py:143-246 (`mytest`) on the device: disparity error statistics, the confusion matrices
// of the three DCA region heads and the accumulation of both into a run state -- three small bandwidth/latency-bound
// launches, nothing returns to the host.  Every result is bitwise reproducible: counts are integers (integer atomics
// or exact in fp64), floating sums are fp64 per-workgroup partials reduced in a fixed order; no floating atomics.
#include "dca_common.h"
#include "../../include/dca_hip.h"

#define EVM_THREADS 256
#define EVM_MAX_BLOCKS 128      // workgroups per image of dca_disp_metrics (= partial records per image)
#define EVM_NREC DCA_EVAL_REC   // doubles per record

// ---- (a) disparity metrics --------------------------------------------------------------------------------------------
// workgroup total of `v` over EVM_THREADS threads in a fixed order (xor butterfly per wave, then waves 0..3 in turn);
// valid in thread 0
__device__ __forceinline__ double evm_block_sum(double v, double* red) {
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();                       // `red` may still be read by the previous call
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// grid (nblk, B): every workgroup walks a fixed, shape-determined set of pixels of one image and writes ONE partial record
__global__ __launch_bounds__(EVM_THREADS) void disp_metrics_partial_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, const unsigned char* __restrict__ mask,
    double* __restrict__ part, int H, int W, int Wp, int top_pad, float maxdisp) {
  __shared__ double red[EVM_THREADS / 64];
  const int b = blockIdx.y, nblk = gridDim.x;
  const long HW = (long)H * W;
  const float* g = gt + b * HW;
  const float* p = pred + (long)b * (H + top_pad) * Wp + (long)top_pad * Wp;   // crop [:, top_pad:, :W] by addressing
  const unsigned char* m = mask ? mask + b * HW : nullptr;
  unsigned n_mask = 0, n_pos = 0, c1 = 0, c2 = 0, c3 = 0, cd1 = 0;            // < 2^32 pixels per thread
  double s_abs = 0.0, s_sl1 = 0.0;
  for (unsigned i = blockIdx.x * EVM_THREADS + threadIdx.x; i < (unsigned)HW; i += (unsigned)nblk * EVM_THREADS) {   // H W < 2^31
    const unsigned r = i / (unsigned)W, c = i - r * (unsigned)W;
    const float gv = g[i];
    n_pos += gv > 0.f;
    const bool in = m ? (m[i] != 0) : (gv > 0.f && gv < maxdisp);
    if (in) {
      const float e = fabsf(p[(long)r * Wp + c] - gv);                       // fp32, as torch evaluates it
      const float sl1 = e < 1.f ? 0.5f * e * e : e - 0.5f;                   // smooth_l1, beta 1
      n_mask += 1;
      s_abs += (double)e;
      s_sl1 += (double)sl1;
      c1 += e > 1.f;
      c2 += e > 2.f;
      c3 += e > 3.f;
      cd1 += (e > 3.f) & (e / fabsf(gv) > 0.05f);
    }
  }
  const double vals[EVM_NREC] = {(double)n_mask, (double)n_pos, s_abs, s_sl1, (double)c1, (double)c2, (double)c3, (double)cd1};
  double* out = part + ((long)b * nblk + blockIdx.x) * EVM_NREC;
#pragma unroll
  for (int k = 0; k < EVM_NREC; ++k) {
    const double t = evm_block_sum(vals[k], red);
    if (threadIdx.x == 0) out[k] = t;
  }
}

// grid B, one wave: lane l adds partials l, l+64, ... in turn, then the butterfly
__global__ __launch_bounds__(64) void disp_metrics_final_kernel(const double* __restrict__ part, double* __restrict__ rec,
                                                                int nblk) {
  const int b = blockIdx.x;
  for (int k = 0; k < EVM_NREC; ++k) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) v += part[((long)b * nblk + i) * EVM_NREC + k];
    v = wave_sum_d(v);
    if (threadIdx.x == 0) rec[b * EVM_NREC + k] = v;
  }
}

static inline int evm_blocks(long HW) {
  long n = (HW + (long)EVM_THREADS * 8 - 1) / ((long)EVM_THREADS * 8);
  return (int)(n < 1 ? 1 : (n > EVM_MAX_BLOCKS ? EVM_MAX_BLOCKS : n));
}

extern "C" long dca_disp_metrics_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (long)B * evm_blocks((long)H * W) * EVM_NREC * (long)sizeof(double);
}

extern "C" int dca_disp_metrics(const float* pred, const float* gt, const unsigned char* mask, double* rec,
                                void* workspace, int B, int H, int W, int top_pad, int right_pad, float maxdisp,
                                hipStream_t stream) {
  DCA_REQUIRE(pred && gt && rec && workspace);
  DCA_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && top_pad >= 0 && right_pad >= 0);
  DCA_REQUIRE((long)(H + top_pad) * (W + right_pad) < (1L << 31));
  const int nblk = evm_blocks((long)H * W);
  disp_metrics_partial_kernel<<<dim3(nblk, B), EVM_THREADS, 0, stream>>>(pred, gt, mask, (double*)workspace, H, W,
                                                                          W + right_pad, top_pad, maxdisp);
  disp_metrics_final_kernel<<<B, 64, 0, stream>>>((const double*)workspace, rec, nblk);
  return dca_launch_status();
}

// ---- (b) region confusion matrices ---------------------------------------------------------------------------------------
// One thread per 1/8-resolution cell (b, i, j): the label (adaptive average pool of gt / 8, floor) once, then the arg-max of
// each volume; LDS histogram per workgroup, non-zero bins flushed with 64-bit integer atomics.
__global__ __launch_bounds__(EVM_THREADS) void region_confusion_kernel(
    const float* __restrict__ v0, const float* __restrict__ v1, const float* __restrict__ v2, const float* __restrict__ gt,
    unsigned long long* __restrict__ cm, int nvol, int B, int C, int hp, int wp, int H, int W) {
  extern __shared__ unsigned hist[];     // nvol * C * C
  const int nbin = nvol * C * C;
  for (int i = threadIdx.x; i < nbin; i += EVM_THREADS) hist[i] = 0;
  __syncthreads();
  const int h = H >> 3, w = W >> 3, roff = hp - h;
  const long cell = (long)blockIdx.x * EVM_THREADS + threadIdx.x;
  if (cell < (long)B * h * w) {
    const int j = (int)(cell % w), i = (int)((cell / w) % h), b = (int)(cell / ((long)w * h));
    // adaptive_avg_pool2d window [floor(i H / h), ceil((i + 1) H / h)): fp32 row-major running sum, ONE division
    const int r0 = (int)(((long)i * H) / h), r1 = (int)((((long)i + 1) * H + h - 1) / h);
    const int q0 = (int)(((long)j * W) / w), q1 = (int)((((long)j + 1) * W + w - 1) / w);
    const float* g = gt + (long)b * H * W;
    float s = 0.f;
    for (int r = r0; r < r1; ++r)
      for (int q = q0; q < q1; ++q) s += g[(long)r * W + q] * 0.125f;       // gt / 8 is exact
    const float lab = floorf(s / (float)((r1 - r0) * (q1 - q0)));
    if (lab >= 0.f && lab < (float)C) {                                       // genConfusionMatrix drops the other labels
      const int label = (int)lab;
      const long plane = (long)hp * wp;
      const long base = (long)b * C * plane + (long)(i + roff) * wp + j;
      for (int k = 0; k < nvol; ++k) {
        const float* v = (k == 0 ? v0 : k == 1 ? v1 : v2) + base;
        float best = v[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
          const float x = v[c * plane];
          if (x > best || (x != x && best == best)) { best = x; arg = c; }   // lowest index on ties; NaN counts as maximum
        }
        atomicAdd(&hist[(k * C + label) * C + arg], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbin; i += EVM_THREADS) {
    const unsigned n = hist[i];
    if (n) atomicAdd(&cm[i], (unsigned long long)n);
  }
}

extern "C" int dca_region_confusion(const float* vol0, const float* vol1, const float* vol2, const float* gt,
                                    long long* cm, int nvol, int B, int C, int hp, int wp, int H, int W,
                                    hipStream_t stream) {
  DCA_REQUIRE(vol0 && gt && cm && nvol >= 1 && nvol <= 3 && (nvol < 2 || vol1) && (nvol < 3 || vol2));
  DCA_REQUIRE(B > 0 && C >= 1 && C <= DCA_EVAL_MAX_CLASSES && H >= 8 && W >= 8);
  DCA_REQUIRE(hp >= (H >> 3) && wp >= (W >> 3));
  DCA_REQUIRE((long)B * C * hp * wp < (1L << 40) && (long)B * H * W < (1L << 40));
  const size_t bytes = (size_t)nvol * C * C * sizeof(long long);
  hipError_t rc = hipMemsetAsync(cm, 0, bytes, stream);
  if (rc != hipSuccess) return (int)rc;
  const long cells = (long)B * (H >> 3) * (W >> 3);
  region_confusion_kernel<<<cdiv(cells, EVM_THREADS), EVM_THREADS, (size_t)nvol * C * C * sizeof(unsigned), stream>>>(
      vol0, vol1, vol2, gt, (unsigned long long*)cm, nvol, B, C, hp, wp, H, W);
  return dca_launch_status();
}

// ---- (c) accumulation into the run state -----------------------------------------------------------------------------------
// One wave.  Lane c owns class c of the (cumulative) confusion matrices; lane 0 owns the scalars.  State layout: dca_hip.h.
__global__ __launch_bounds__(64) void eval_accumulate_kernel(const double* __restrict__ rec, const long long* __restrict__ cm,
                                                             double* __restrict__ state, int B, int nvol, int C, long npix) {
  const int c = threadIdx.x;
  const int CC = C * C;
  // the reference never resets its SegmentationMetric between the heads (main_dca.py:215-232): head k is scored on
  // CM0 + ... + CMk
  double mpa[3], miou[3];
  long long row = 0, col = 0, diag = 0;
  for (int k = 0; k < 3; ++k) {
    if (k < nvol && c < C) {
      const long long* m = cm + (long)k * CC;
      for (int x = 0; x < C; ++x) {
        row += m[c * C + x];
        col += m[x * C + c];
      }
      diag += m[c * C + c];
    }
    // np.nanmean over classes: 0/0 classes are left out (fp64 division of exact integers, as numpy does it)
    const long long uni = row + col - diag;
    const double acc = (c < C && row > 0) ? (double)diag / (double)row : 0.0;
    const double iou = (c < C && uni > 0) ? (double)diag / (double)uni : 0.0;
    const double nacc = wave_sum_d((c < C && row > 0) ? 1.0 : 0.0), niou = wave_sum_d((c < C && uni > 0) ? 1.0 : 0.0);
    mpa[k] = wave_sum_d(acc) / nacc;        // 0/0 = NaN when no class is present, as np.nanmean
    miou[k] = wave_sum_d(iou) / niou;
  }
  // per-head matrices of the run, NOT accumulated over the heads
  for (int i = c; i < nvol * CC; i += 64) state[DCA_EVAL_STATE_HEAD + i] += (double)cm[i];
  if (c != 0) return;
  double n = 0, s_abs = 0, s_sl1 = 0, c1 = 0, c3 = 0;
  for (int b = 0; b < B; ++b) {
    const double* r = rec + b * EVM_NREC;
    n += r[0]; s_abs += r[2]; s_sl1 += r[3]; c1 += r[4]; c3 += r[6];
    // utils/metrics.py: images whose mask covers < 10 % of their positive ground truth are skipped (fp32, as there);
    // an image without any masked pixel is skipped too (its mean would be NaN)
    const float fm = (float)r[0] / (float)npix, fp = (float)r[1] / (float)npix;
    if (r[0] > 0 && !(fm / fp < 0.1f)) {
      state[DCA_EVAL_IMG_KEPT] += 1.0;
      state[DCA_EVAL_IMG_EPE] += r[2] / r[0];
      state[DCA_EVAL_IMG_D1] += r[7] / r[0];
      state[DCA_EVAL_IMG_THRES + 0] += r[4] / r[0];
      state[DCA_EVAL_IMG_THRES + 1] += r[5] / r[0];
      state[DCA_EVAL_IMG_THRES + 2] += r[6] / r[0];
    }
    state[DCA_EVAL_IMG_SEEN] += 1.0;
  }
  state[DCA_EVAL_PIXELS] += n;
  state[DCA_EVAL_BATCHES] += 1.0;
  if (n > 0) {                               // an empty mask makes all ten values 0 for the batch, which still counts
    state[DCA_EVAL_SUMS + 0] += s_sl1 / n;
    state[DCA_EVAL_SUMS + 1] += s_abs / n;
    state[DCA_EVAL_SUMS + 2] += c1 / n;
    state[DCA_EVAL_SUMS + 3] += c3 / n;
    for (int k = 0; k < 3; ++k) {
      state[DCA_EVAL_SUMS + 4 + k] += mpa[k];
      state[DCA_EVAL_SUMS + 7 + k] += miou[k];
    }
  }
}

extern "C" long dca_eval_state_len(int C) {
  if (C < 1 || C > DCA_EVAL_MAX_CLASSES) return 0;
  return DCA_EVAL_STATE_HEAD + 3L * C * C;
}

extern "C" int dca_eval_accumulate(const double* rec, const long long* cm, double* state, int B, int nvol, int C,
                                   int H, int W, hipStream_t stream) {
  DCA_REQUIRE(rec && cm && state && B > 0 && nvol >= 1 && nvol <= 3 && C >= 1 && C <= DCA_EVAL_MAX_CLASSES);
  DCA_REQUIRE(H > 0 && W > 0);
  eval_accumulate_kernel<<<1, 64, 0, stream>>>(rec, cm, state, B, nvol, C, (long)H * W);
  return dca_launch_status();
}
