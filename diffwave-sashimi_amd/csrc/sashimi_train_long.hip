// Training kernels of the S4 blocks whose stage runs on rocFFT instead of the fused LDS convolution: odd stage lengths and
// stages longer than 16384 samples (`configs/experiment/ljspeech_harder.yaml`: L = 44000).  Everything here streams; the
// transforms themselves are rocFFT plans driven from sashimi_model.hip (n = 2L, batched over the B H rows).
//
// Forward:   a = C2R(R2C(u) K_f) / 2L + D u,  g = gelu(a)                    (s4.py:1403-1430)
// Backward:  du  = C2R(conj(K_f) dA) / 2L + D da                              (the convolution's adjoint)
//            dK_f = sum_b conj(U_b) dA_b,  dK = C2R(dK_f) / 2L                (the tap gradient: lag-j correlation of u and da)
//            dk = the two-sided assembly (s4_twosided_kernel) backwards, dD = dK[0] = sum u da
// U and dA are the 2L-point spectra of the zero-padded rows of u and da.
#include "sashimi_train.h"

namespace dws {

__device__ __forceinline__ float2 cmulc_l(float2 a, float2 b) {  // conj(a) * b
    return make_float2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}

// out[row][j] = j < L ? in[row][j] : 0,  j < 2L: unpadded rows into the zero-padded rows the R2C reads
__global__ void pad_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int L) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t row = blockIdx.y;
    if (j >= 2 * L) return;
    out[row * 2 * L + j] = j < L ? in[row * L + j] : 0.f;
}

int launch_pad_rows(const float* in, float* out, int rows, int L, hipStream_t s) {
    DWS_CHECK(rows > 0 && rows <= 65535 && L > 0, DWS_ERR_UNSUPPORTED, "pad_rows: %d rows of %d", rows, L);
    ProfileScope ps("pad_rows", s);
    hipLaunchKernelGGL(pad_rows_kernel, dim3(ceil_div(2 * L, 256), rows), dim3(256), 0, s, in, out, L);
    return DWS_OK;
}

// a = yc / 2L + D[h] u;  pre = a, g = gelu(a).  The sampling path's s4_post with the pre-activation kept for the backward
// (gelu'(a) of the output projection's adjoint); u is the unpadded row, yc the C2R output row of length 2L.
__global__ void s4_post_train_kernel(const float* __restrict__ yc, const float* __restrict__ u, const float* __restrict__ D,
                                     float* __restrict__ pre, float* __restrict__ g, int H, int L) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    const int h = blockIdx.y, b = blockIdx.z;
    if (l >= L) return;
    const size_t row = (size_t)b * H + h;
    const float a = yc[row * 2 * L + l] * (1.f / (float)(2 * L)) + u[row * L + l] * D[h];
    pre[row * L + l] = a;
    g[row * L + l] = dws_gelu(a);
}

int launch_s4_post_train(const float* yc, const float* u, const float* D, float* pre, float* g, int B, int H, int L,
                         hipStream_t s) {
    DWS_CHECK(B > 0 && B <= 65535 && H > 0 && H <= 65535 && L > 0, DWS_ERR_UNSUPPORTED, "s4_post_train: B=%d H=%d", B, H);
    ProfileScope ps("s4_post_train", s);
    hipLaunchKernelGGL(s4_post_train_kernel, dim3(ceil_div(L, 256), H, B), dim3(256), 0, s, yc, u, D, pre, g, H, L);
    return DWS_OK;
}

// Spectral part of the convolution's adjoint, one pass over the spectra (thread = one bin k of one channel h):
//   dkf[h][k] = sum_b conj(uf[b][h][k]) daf[b][h][k]      (b in order: no atomics, run-to-run identical bits)
//   daf[b][h][k] *= conj(kf[h][k])                         (in place: the C2R that follows gives the data gradient)
__global__ void conv_adjoint_spec_kernel(const float2* __restrict__ uf, float2* __restrict__ daf, const float2* __restrict__ kf,
                                         float2* __restrict__ dkf, int B, int H, int Lf) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int h = blockIdx.y;
    if (k >= Lf) return;
    const float2 kk = kf[(size_t)h * Lf + k];
    float2 acc = make_float2(0.f, 0.f);
    for (int b = 0; b < B; ++b) {
        const size_t i = ((size_t)b * H + h) * Lf + k;
        const float2 d = daf[i];
        const float2 p = cmulc_l(uf[i], d);
        acc.x += p.x;
        acc.y += p.y;
        daf[i] = cmulc_l(kk, d);
    }
    dkf[(size_t)h * Lf + k] = acc;
}

// The data half of it alone (data-only backward): daf[b][h][k] *= conj(kf[h][k]), the same product.
__global__ void conv_adjoint_spec_data_kernel(float2* __restrict__ daf, const float2* __restrict__ kf, int B, int H, int Lf) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int h = blockIdx.y;
    if (k >= Lf) return;
    const float2 kk = kf[(size_t)h * Lf + k];
    for (int b = 0; b < B; ++b) {
        const size_t i = ((size_t)b * H + h) * Lf + k;
        daf[i] = cmulc_l(kk, daf[i]);
    }
}

int launch_conv_adjoint_spec_data(float* daf, const float* kf, int B, int H, int Lf, hipStream_t s) {
    DWS_CHECK(B > 0 && H > 0 && H <= 65535 && Lf > 0, DWS_ERR_UNSUPPORTED, "conv_adjoint_spec: B=%d H=%d", B, H);
    ProfileScope ps("conv_adjoint_spec_data", s);
    hipLaunchKernelGGL(conv_adjoint_spec_data_kernel, dim3(ceil_div(Lf, 256), H), dim3(256), 0, s, (float2*)daf, (const float2*)kf,
                       B, H, Lf);
    return DWS_OK;
}

int launch_conv_adjoint_spec(const float* uf, float* daf, const float* kf, float* dkf, int B, int H, int Lf, hipStream_t s) {
    DWS_CHECK(B > 0 && H > 0 && H <= 65535 && Lf > 0, DWS_ERR_UNSUPPORTED, "conv_adjoint_spec: B=%d H=%d", B, H);
    ProfileScope ps("conv_adjoint_spec", s);
    hipLaunchKernelGGL(conv_adjoint_spec_kernel, dim3(ceil_div(Lf, 256), H), dim3(256), 0, s, (const float2*)uf, (float2*)daf,
                       (const float2*)kf, (float2*)dkf, B, H, Lf);
    return DWS_OK;
}

// du[b][h][l] = yc[b][h][l] / 2L + D[h] da[b][h][l]   (yc: C2R rows of length 2L)
// rowsum[b * rs_bstride + h] = sum_l du[b][h][l]        (d fc_t(e): u = LN1(x) + fc_t(e); one workgroup per row, fixed order)
__global__ __launch_bounds__(256) void conv_adjoint_epi_kernel(const float* __restrict__ yc, const float* __restrict__ da,
                                                               const float* __restrict__ D, float* __restrict__ du,
                                                               float* __restrict__ rowsum, int rs_bstride, int H, int L) {
    __shared__ float red[4];
    const int h = blockIdx.x, b = blockIdx.y;
    const size_t row = (size_t)b * H + h;
    const float inv = 1.f / (float)(2 * L), dh = D[h];
    const float* __restrict__ y = yc + row * 2 * L;
    const float* __restrict__ d = da + row * L;
    float* __restrict__ o = du + row * L;
    float acc = 0.f;
    for (int l = threadIdx.x; l < L; l += 256) {
        const float v = y[l] * inv + dh * d[l];
        o[l] = v;
        acc += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (rowsum && threadIdx.x == 0) rowsum[(size_t)b * rs_bstride + h] = red[0] + red[1] + red[2] + red[3];
}

int launch_conv_adjoint_epi(const float* yc, const float* da, const float* D, float* du, float* rowsum, int rs_bstride, int B,
                            int H, int L, hipStream_t s) {
    DWS_CHECK(B > 0 && B <= 65535 && H > 0 && L > 0, DWS_ERR_UNSUPPORTED, "conv_adjoint_epi: B=%d H=%d", B, H);
    ProfileScope ps("conv_adjoint_epi", s);
    hipLaunchKernelGGL(conv_adjoint_epi_kernel, dim3(H, B), dim3(256), 0, s, yc, da, D, du, rowsum, rs_bstride, H, L);
    return DWS_OK;
}

// Adjoint of s4_twosided_kernel (K[h][j] = k0[h][j] / Lk for j < Lt, K[h][2L-1-i] = k1[h][i] / Lk for i < Lt), given the
// unnormalised C2R rows dK [H][2L] of the tap gradient:
//   dk[c][h][j] = j < Lt ? dK[h][c ? 2L-1-j : j] * sc : 0   for j < Lk      (sc = 1 / (2L Lk))
//   dD[h] = dK[h][0] * scD                                                  (scD = 1 / 2L: lag 0 of the correlation, sum u da)
__global__ void s4_twosided_bwd_kernel(const float* __restrict__ dK, float* __restrict__ dk, float* __restrict__ dD, int H,
                                       int L, int Lk, int Lt, float sc, float scD) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int h = blockIdx.y;
    if (j >= Lk) return;
    const float* r = dK + (size_t)h * 2 * L;
    const bool in = j < Lt;
    dk[(size_t)h * Lk + j] = in ? r[j] * sc : 0.f;
    dk[((size_t)H + h) * Lk + j] = in ? r[2 * L - 1 - j] * sc : 0.f;
    if (j == 0) dD[h] = r[0] * scD;
}

int launch_s4_twosided_bwd(const float* dK, float* dk, float* dD, int H, int L, int Lk, int Lt, float sc, float scD,
                           hipStream_t s) {
    DWS_CHECK(H > 0 && H <= 65535 && Lk > 0 && Lt <= Lk && Lt <= L, DWS_ERR_UNSUPPORTED, "s4_twosided_bwd: H=%d L=%d Lk=%d Lt=%d",
              H, L, Lk, Lt);
    ProfileScope ps("s4_twosided_bwd", s);
    hipLaunchKernelGGL(s4_twosided_bwd_kernel, dim3(ceil_div(Lk, 256), H), dim3(256), 0, s, dK, dk, dD, H, L, Lk, Lt, sc, scD);
    return DWS_OK;
}

}  // namespace dws
