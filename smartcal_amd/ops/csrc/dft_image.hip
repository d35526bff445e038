// Exact direct-Fourier-sum imager — coherency.hip run in the other
// direction: visibility samples → image pixels.
//
//   I[f, j, y, x] = Σ_s Re[ V[f, j, s] · exp(−2πi (u_s·l_x + v_s·m_y
//                                               + w_s·(n_xy − 1))) ]
//   l_x = l_c + (x − npix/2)·cell_f,  m_y = m_c + (y − npix/2)·cell_f,
//   n_xy = sqrt(1 − l_x² − m_y²),  (u, v, w) = uvw_metres · scale_f.
//
// Weights and the 1/Σg normalisation are folded into V host-side; a
// dropped w-term is a zeroed w column. Pixels beyond the unit circle are 0.
//
// dft_image_kernel: ONE launch for the whole (F, M) cube. Grid (pixel
// tiles × frequencies × sample splits); a 256-thread block owns a 16×16
// pixel tile of one frequency, each thread one pixel. Samples are staged
// through LDS in chunks of DFT_CHUNK: u, v, w in wavelengths (f64) and the
// values of up to DFT_MAPS maps (complex64). Every lane reads the same LDS
// word (broadcast). The phase is formed in cycles in f64 — it reaches 1e5
// at LOFAR scale, where f32 keeps no fraction — reduced to [−½, ½] and
// only then handed to the f32 sincospi; it is computed once per (pixel,
// sample) and shared by the maps of a group. Accumulation is f64.
//
// 128² pixels are only 64 tiles per frequency, so blockIdx.z splits the
// sample range into contiguous slices. With one slice the kernel stores
// f32 directly; otherwise it stores f64 partial images that
// dft_image_reduce_kernel adds in slice order — no atomics, so the result
// is bit-identical from run to run.

#include "common.h"

#define DFT_TILE 16
#define DFT_CHUNK 256   // samples per LDS pass: 6 KB uvw + ≤ 8 KB values
#define DFT_MAPS 4      // maps whose accumulators live in registers

namespace {

template <int NM>
__device__ __forceinline__ void dft_group(
    const double* __restrict__ UVW, const float2* __restrict__ V, long S,
    long s_lo, long s_hi, double scale, double l, double m, double nm1,
    double* __restrict__ suvw, float2* __restrict__ sval, double* acc) {
#pragma unroll
  for (int j = 0; j < NM; ++j) acc[j] = 0.0;
  for (long c0 = s_lo; c0 < s_hi; c0 += DFT_CHUNK) {
    const int cn = (int)min((long)DFT_CHUNK, s_hi - c0);
    for (int i = threadIdx.x; i < cn * 3; i += blockDim.x)
      suvw[i] = scale * UVW[c0 * 3 + i];
    for (int i = threadIdx.x; i < cn * NM; i += blockDim.x) {
      const int j = i / cn, s = i - j * cn;      // consecutive s per map
      sval[s * NM + j] = V[(long)j * S + c0 + s];
    }
    __syncthreads();
    for (int s = 0; s < cn; ++s) {
      const double ph = suvw[3 * s] * l + suvw[3 * s + 1] * m
                        + suvw[3 * s + 2] * nm1;
      const float r = (float)(ph - rint(ph));    // cycles in [−½, ½]
      float sn, cs;
      sincospif(2.0f * r, &sn, &cs);
#pragma unroll
      for (int j = 0; j < NM; ++j) {
        const float2 val = sval[s * NM + j];
        // Re[V · e^{−iφ}] = Vr·cosφ + Vi·sinφ
        acc[j] += (double)(val.x * cs + val.y * sn);
      }
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void dft_image_kernel(
    const double* __restrict__ UVW,   // (S, 3) metres
    const float2* __restrict__ V,     // (F, M, S) pre-weighted complex64
    const double* __restrict__ FP,    // (F, 2): scale = f/c, cell
    float* __restrict__ OUT,          // (F, M, npix, npix), one slice
    double* __restrict__ PART,        // (nsplit, F, M, npix, npix) or null
    double lc, double mc, long S, int M, int npix, int F, int nsplit) {
  __shared__ double suvw[DFT_CHUNK * 3];
  __shared__ float2 sval[DFT_CHUNK * DFT_MAPS];
  const int ntx = (npix + DFT_TILE - 1) / DFT_TILE;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int x = tx * DFT_TILE + (threadIdx.x & (DFT_TILE - 1));
  const int y = ty * DFT_TILE + (threadIdx.x / DFT_TILE);
  const int f = blockIdx.y, z = blockIdx.z;
  const bool live = x < npix && y < npix;

  const double scale = FP[2 * f], cell = FP[2 * f + 1];
  const double l = lc + (double)(x - npix / 2) * cell;
  const double m = mc + (double)(y - npix / 2) * cell;
  const double r2 = l * l + m * m;
  const bool sky = r2 <= 1.0;
  // n − 1 without cancellation near the centre
  const double nm1 = sky ? -r2 / (1.0 + sqrt(1.0 - r2)) : 0.0;

  const long s_lo = S * z / nsplit, s_hi = S * (z + 1) / nsplit;
  const long plane = (long)npix * npix;
  for (int g = 0; g < M; g += DFT_MAPS) {
    const int nm = min(DFT_MAPS, M - g);
    const float2* Vg = V + ((long)f * M + g) * S;
    double acc[DFT_MAPS];
    switch (nm) {   // uniform over the block
      case 1: dft_group<1>(UVW, Vg, S, s_lo, s_hi, scale, l, m, nm1, suvw,
                           sval, acc); break;
      case 2: dft_group<2>(UVW, Vg, S, s_lo, s_hi, scale, l, m, nm1, suvw,
                           sval, acc); break;
      case 3: dft_group<3>(UVW, Vg, S, s_lo, s_hi, scale, l, m, nm1, suvw,
                           sval, acc); break;
      default: dft_group<4>(UVW, Vg, S, s_lo, s_hi, scale, l, m, nm1, suvw,
                            sval, acc); break;
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < DFT_MAPS; ++j) {
        if (j >= nm) break;
        const double a = sky ? acc[j] : 0.0;
        const long o = ((long)f * M + g + j) * plane + (long)y * npix + x;
        if (PART) PART[(long)z * F * M * plane + o] = a;
        else OUT[o] = (float)a;
      }
    }
  }
}

// OUT[i] = (float) Σ_z PART[z, i], z ascending.
extern "C" __global__ __launch_bounds__(256) void dft_image_reduce_kernel(
    const double* __restrict__ PART, float* __restrict__ OUT, long n,
    int nsplit) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (int z = 0; z < nsplit; ++z) a += PART[(long)z * n + i];
  OUT[i] = (float)a;
}
