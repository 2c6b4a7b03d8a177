// Spectral templates of the linear mixing model: the median filter along lambda and the coordinate-descent NMF of the
// reference's template notebooks (scipy.ndimage.median_filter(cube, size, axes=[0]) and
// sklearn.decomposition.NMF(solver="cd"), sklearn 1.7 _fit_coordinate_descent / _update_cdnmf_fast).
//
// Median: one thread per column of a C-order [L][C] array slides a window of `size` values along axis 0.  The window
// sits at the end of a register array of SMAX entries (SMAX a compile-time bucket >= size, the leading SMAX - size
// entries are +inf), so every register index is a constant.  The output is the value of rank size / 2 of the window,
// selected by counting (#less <= rank < #less-or-equal): one of the inputs, exactly, as scipy's rank filter returns.
// Out-of-range rows fold as scipy's NI_ExtendLine does (reflect, nearest, mirror), also for windows longer than L.
//
// NMF: n_models models share one X [P][L].  Their H are stacked as Hcat [N][L] (N = sum K) and their W as
// Wcat [P][N]; one iteration is
//   XHt = X Hcat^T (split over L, partial sums added in a fixed order), HHt = Hcat Hcat^T,
//   W sweep: thread per (model, row), components in order, sklearn's float arithmetic (no contraction),
//   WtX = Wcat^T X, WtW = Wcat^T Wcat,
//   H sweep: thread per (model, column),
//   finalize: violation = sum |projected gradient| (float64, fixed-order tree), sklearn's stopping test.
// A model's converged flag lives on the device; a set flag turns its later queued sweeps into no-ops, so the host only
// polls every few iterations.  Every output element of the GEMMs is reduced in an order that depends on (P, L) alone,
// so a model gives the same bits whatever else shares its batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/surfh_amd.h"
#include "dev_buf.h"

using surfh_impl::DevBuf;

namespace {

thread_local std::string g_tmpl_err;
int tfail(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_tmpl_err = buf;
    return 1;
}
#define T_OK(x)                                                                                    \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) return tfail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define T_ALLOC(expr)                                                                              \
    do {                                                                                           \
        if (expr) return tfail("%s", surfh_last_error());       /* the allocator's message, in this module's error string */ \
    } while (0)

// ---------------------------------------------------------------------------------------------------------------------
// spectral median

// scipy.ndimage's boundary extension (NI_ExtendLine), written as a fold of any index onto [0, L)
__device__ __forceinline__ long fold_index(long j, long L, int mode) {
    if (j >= 0 && j < L) return j;
    if (mode == 1) return j < 0 ? 0 : L - 1;                   // nearest
    if (mode == 0) {                                           // reflect: d c b a | a b c d | d c b a
        const long p = 2 * L;
        long k = j % p;
        if (k < 0) k += p;
        return k < L ? k : p - 1 - k;
    }
    if (L == 1) return 0;                                      // mirror: d c b | a b c d | c b a
    const long p = 2 * L - 2;
    long k = j % p;
    if (k < 0) k += p;
    return k < L ? k : p - k;
}

template <int SMAX>
__global__ __launch_bounds__(256) void k_median(const float *__restrict__ src, float *__restrict__ dst, long L, long C,
                                                int size, int mode) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int rank = size / 2;
    const long left = size / 2;                                // window of output l: rows l - left .. l - left + size - 1
    float w[SMAX];
#pragma unroll
    for (int k = 0; k < SMAX; ++k) {
        const int q = k - (SMAX - size);                       // position in the window
        w[k] = q < 0 ? INFINITY : src[fold_index(q - left, L, mode) * C + c];
    }
    for (long l = 0; l < L; ++l) {
        if (l > 0) {                                           // slide: drop the oldest, append row l - left + size - 1
#pragma unroll
            for (int k = 0; k < SMAX - 1; ++k) w[k] = (k < SMAX - size) ? INFINITY : w[k + 1];
            w[SMAX - 1] = src[fold_index(l - left + size - 1, L, mode) * C + c];
        }
        float med = 0.f;
#pragma unroll
        for (int a = 0; a < SMAX; ++a) {                       // a padding entry (+inf) has #less = size > rank
            int lt = 0, le = 0;
#pragma unroll
            for (int b = 0; b < SMAX; ++b) {
                lt += w[b] < w[a];
                le += w[b] <= w[a];
            }
            if (lt <= rank && rank < le) med = w[a];
        }
        dst[l * C + c] = med;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// NMF

constexpr int GT = 64;           // GEMM tile (both output dimensions)
constexpr int GK = 16;           // GEMM k step
constexpr int KCHUNK = 512;      // split of the reduction of gemm_nt (depends on nothing but the reduction length)
constexpr int RED = 256;

// part[s][m][n] = sum_{k in chunk s} A[m][k] B[n][k]     A [M][Kd], B [N][Kd]
__global__ __launch_bounds__(256) void k_gemm_nt(const float *__restrict__ A, const float *__restrict__ B,
                                                 float *__restrict__ part, int M, int N, long Kd) {
    __shared__ float As[GK][GT + 4], Bs[GK][GT + 4];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const int m0 = blockIdx.x * GT, n0 = blockIdx.y * GT;
    const long k0 = (long)blockIdx.z * KCHUNK, k1 = std::min<long>(k0 + KCHUNK, Kd);
    float acc[4][4] = {};
    for (long kb = k0; kb < k1; kb += GK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = t + 256 * e, r = idx / GK, kk = idx % GK;
            const long k = kb + kk;
            As[kk][r] = (m0 + r < M && k < k1) ? A[(long)(m0 + r) * Kd + k] : 0.f;
            Bs[kk][r] = (n0 + r < N && k < k1) ? B[(long)(n0 + r) * Kd + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[kk][ty * 4 + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tx * 4 + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
    float *o = part + (long)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n < N) o[(long)m * N + n] = acc[i][j];
        }
    }
}

// C[i] = sum_s part[s][i], s ascending
__global__ void k_sum_parts(const float *__restrict__ part, float *__restrict__ Cm, long MN, int S) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MN) return;
    float s = part[i];
    for (int k = 1; k < S; ++k) s += part[(long)k * MN + i];
    Cm[i] = s;
}

// C[m][n] = sum_p A[p][m] B[p][n], p ascending     A [Kd][M], B [Kd][N]
__global__ __launch_bounds__(256) void k_gemm_tn(const float *__restrict__ A, const float *__restrict__ B,
                                                 float *__restrict__ Cm, int M, long N, long Kd) {
    __shared__ float As[GK][GT + 4], Bs[GK][GT + 4];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const long m0 = (long)blockIdx.y * GT, n0 = (long)blockIdx.x * GT;
    float acc[4][4] = {};
    for (long kb = 0; kb < Kd; kb += GK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = t + 256 * e, kk = idx / GT, r = idx % GT;
            const long k = kb + kk;
            As[kk][r] = (m0 + r < M && k < Kd) ? A[k * M + m0 + r] : 0.f;
            Bs[kk][r] = (n0 + r < N && k < Kd) ? B[k * N + n0 + r] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[kk][ty * 4 + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tx * 4 + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long m = m0 + ty * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long n = n0 + tx * 4 + j;
            if (n < N) Cm[m * N + n] = acc[i][j];
        }
    }
}

struct Model {
    int off, K;                  // columns [off, off + K) of Wcat / rows of Hcat
};

#pragma clang fp contract(off)
// One coordinate sweep of _update_cdnmf_fast for every (model, row): V [rows][ldv] holds the rows being updated
// (columns off..off+K of row i, stride sv between the K entries), G the Gram matrix [N][N], R the cross product
// (entry t of row i at R[i * r_row + (off + t) * r_col]).  The float arithmetic is sklearn's, in its order.
__global__ void k_sweep(const Model *__restrict__ models, int n_models, const int *__restrict__ done,
                        float *__restrict__ V, long rows, long v_row, long v_col, const float *__restrict__ G, int N,
                        const float *__restrict__ R, long r_row, long r_col, double *__restrict__ viol) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (i >= rows || done[m]) return;
    const int off = models[m].off, K = models[m].K;
    double v = 0.0;
    for (int t = 0; t < K; ++t) {
        const float *g = G + (long)(off + t) * N + off;
        float grad = -R[i * r_row + (off + t) * r_col];
        for (int r = 0; r < K; ++r) grad = __fadd_rn(grad, __fmul_rn(g[r], V[i * v_row + (off + r) * v_col]));
        float &w = V[i * v_row + (off + t) * v_col];
        const float pg = w == 0.f ? fminf(0.f, grad) : grad;
        v += (double)fabsf(pg);
        const float hess = g[t];
        if (hess != 0.f) w = fmaxf(__fsub_rn(w, __fdiv_rn(grad, hess)), 0.f);
    }
    viol[(long)m * rows + i] = v;
}
#pragma clang fp contract(on)

// fixed-order sum of x[0..n) by one block of RED threads (thread j takes j, j + RED, ...; then a tree)
__device__ double block_sum(const double *__restrict__ x, long n) {
    __shared__ double red[RED];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += RED) s += x[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = RED / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// sklearn's stopping test after iteration `it` (1-based), one block per model
__global__ __launch_bounds__(RED) void k_finalize(int *__restrict__ done, int *__restrict__ n_iter,
                                                  double *__restrict__ vinit, double *__restrict__ trace,
                                                  const double *__restrict__ vw, long P, const double *__restrict__ vh,
                                                  long L, int it, int max_iter, double tol) {
    const int m = blockIdx.x;
    if (done[m]) return;
    const double v = block_sum(vw + (long)m * P, P) + block_sum(vh + (long)m * L, L);
    if (threadIdx.x) return;
    trace[(long)m * max_iter + it - 1] = v;
    if (it == 1) vinit[m] = v;
    const double v0 = vinit[m];
    if (v0 == 0.0 || v / v0 <= tol || it == max_iter) {
        done[m] = 1;
        n_iter[m] = it;
    }
}

// per block and model: sum over its elements of (x - wh)^2 and of (x - wh) / x (x != 0), wh = W H in float64
constexpr int ERR_ROWS = 8;
__global__ __launch_bounds__(RED) void k_recon(const Model *__restrict__ models, int n_models,
                                               const float *__restrict__ X, const float *__restrict__ Wcat,
                                               const float *__restrict__ Hcat, long P, long L, int N,
                                               double *__restrict__ part) {
    const long nbl = (L + RED - 1) / RED, b = blockIdx.x, nb = gridDim.x;      // block b: columns of b % nbl, rows of b / nbl
    const long l = (b % nbl) * RED + threadIdx.x;
    const long i0 = (b / nbl) * ERR_ROWS;
    __shared__ double red[2][RED];
    for (int m = 0; m < n_models; ++m) {
        const int off = models[m].off, K = models[m].K;
        double s2 = 0.0, sr = 0.0;
        if (l < L) {
            for (long i = i0; i < std::min(i0 + ERR_ROWS, P); ++i) {
                const double x = X[i * L + l];
                double wh = 0.0;
                for (int k = 0; k < K; ++k) wh += (double)Wcat[i * N + off + k] * (double)Hcat[(long)(off + k) * L + l];
                const double r = x - wh;
                s2 += r * r;
                if (x != 0.0) sr += r / x;
            }
        }
        red[0][threadIdx.x] = s2;
        red[1][threadIdx.x] = sr;
        __syncthreads();
        for (int h = RED / 2; h > 0; h >>= 1) {
            if (threadIdx.x < h) {
                red[0][threadIdx.x] += red[0][threadIdx.x + h];
                red[1][threadIdx.x] += red[1][threadIdx.x + h];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            part[((long)m * 2 + 0) * nb + b] = red[0][0];
            part[((long)m * 2 + 1) * nb + b] = red[1][0];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RED) void k_recon_final(const double *__restrict__ part, long nb, double *__restrict__ out) {
    const int m = blockIdx.x;
    const double s2 = block_sum(part + (long)m * 2 * nb, nb);
    const double sr = block_sum(part + ((long)m * 2 + 1) * nb, nb);
    if (threadIdx.x == 0) {
        out[m * 2 + 0] = sqrt(s2);
        out[m * 2 + 1] = sr;
    }
}

inline unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

extern "C" {

const char *surfh_templates_last_error(void) { return g_tmpl_err.c_str(); }

int surfh_spectral_median(const float *src, float *dst, int64_t L, int64_t C, int32_t size, int32_t mode,
                          int32_t device) {
    if (!src || !dst || L < 1 || C < 0) return tfail("surfh_spectral_median: bad arguments");
    if (size < 1 || size > 63) return tfail("surfh_spectral_median: size %d outside 1..63", size);
    if (mode < 0 || mode > 2) return tfail("surfh_spectral_median: mode %d is not reflect (0), nearest (1) or mirror (2)", mode);
    if (C == 0) return 0;
    T_OK(hipSetDevice(device));
    const size_t n = (size_t)L * (size_t)C;
    DevBuf<float> ds, dd;
    T_ALLOC(ds.alloc(n) || dd.alloc(n));
    T_OK(hipMemcpy(ds, src, n * 4, hipMemcpyHostToDevice));
    const dim3 grid(cdiv(C, 256)), block(256);
    if (size <= 8) k_median<8><<<grid, block>>>(ds, dd, L, C, size, mode);
    else if (size <= 16) k_median<16><<<grid, block>>>(ds, dd, L, C, size, mode);
    else if (size <= 32) k_median<32><<<grid, block>>>(ds, dd, L, C, size, mode);
    else k_median<64><<<grid, block>>>(ds, dd, L, C, size, mode);
    T_OK(hipGetLastError());
    T_OK(hipMemcpy(dst, dd, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int surfh_nmf_cd(const float *X, int64_t P, int64_t L, int32_t n_models, const int32_t *K, float *W, float *H,
                 int32_t max_iter, double tol, int32_t *n_iter, double *violation_trace, double *recon_err, double *mre,
                 int32_t device, float *ms_per_iter) {
    if (!X || !K || !W || !H || !n_iter || P < 1 || L < 1 || n_models < 1 || max_iter < 0)
        return tfail("surfh_nmf_cd: bad arguments");
    std::vector<Model> models(n_models);
    int N = 0;
    for (int m = 0; m < n_models; ++m) {
        if (K[m] < 1) return tfail("surfh_nmf_cd: model %d has %d components", m, K[m]);
        models[m] = Model{N, K[m]};
        N += K[m];
    }
    if (N > 4096) return tfail("surfh_nmf_cd: %d components in all (at most 4096)", N);
    T_OK(hipSetDevice(device));
    // W blocks [P][K_m] one after the other -> Wcat [P][N]; H blocks [K_m][L] are already Hcat [N][L]
    std::vector<float> wcat((size_t)P * N);
    for (int m = 0; m < n_models; ++m) {
        const float *wm = W + (size_t)P * models[m].off;
        for (long i = 0; i < P; ++i)
            for (int k = 0; k < models[m].K; ++k) wcat[(size_t)i * N + models[m].off + k] = wm[(size_t)i * models[m].K + k];
    }
    const int S = (int)cdiv(L, KCHUNK);                    // X Hcat^T and Hcat Hcat^T both reduce over L
    DevBuf<float> dX, dW, dH, xht, hht, wtx, wtw, part;
    DevBuf<double> vw, vh, vinit, trace, rpart, rout;
    DevBuf<int> done, dnit;
    DevBuf<Model> dmod;
    T_ALLOC(dX.alloc((size_t)P * L) || dW.alloc((size_t)P * N) || dH.alloc((size_t)N * L) || xht.alloc((size_t)P * N) ||
            hht.alloc((size_t)N * N) || wtx.alloc((size_t)N * L) || wtw.alloc((size_t)N * N) ||
            part.alloc((size_t)S * std::max<long>(P, N) * N) || vw.alloc((size_t)n_models * P) || vh.alloc((size_t)n_models * L) ||
            vinit.alloc(n_models) || trace.alloc((size_t)n_models * std::max(max_iter, 1)) || done.alloc(n_models) ||
            dnit.alloc(n_models) || dmod.alloc(n_models));
    T_OK(hipMemcpy(dX, X, (size_t)P * L * 4, hipMemcpyHostToDevice));
    T_OK(hipMemcpy(dW, wcat.data(), (size_t)P * N * 4, hipMemcpyHostToDevice));
    T_OK(hipMemcpy(dH, H, (size_t)N * L * 4, hipMemcpyHostToDevice));
    T_OK(hipMemcpy(dmod, models.data(), n_models * sizeof(Model), hipMemcpyHostToDevice));
    T_OK(hipMemset(done, 0, n_models * sizeof(int)));
    T_OK(hipMemset(dnit, 0, n_models * sizeof(int)));
    T_OK(hipMemset(trace, 0, (size_t)n_models * std::max(max_iter, 1) * sizeof(double)));

    hipEvent_t e0, e1;
    T_OK(hipEventCreate(&e0));
    T_OK(hipEventCreate(&e1));
    T_OK(hipEventRecord(e0, 0));
    const int POLL = 8;
    int it = 1;
    std::vector<int> hdone(n_models);
    for (; it <= max_iter; ++it) {
        // W sweep: XHt = X Hcat^T [P][N], HHt = Hcat Hcat^T [N][N]
        k_gemm_nt<<<dim3(cdiv(P, GT), cdiv(N, GT), S), 256>>>(dX, dH, part, (int)P, N, L);
        k_sum_parts<<<cdiv(P * N, 256), 256>>>(part, xht, P * N, S);
        k_gemm_nt<<<dim3(cdiv(N, GT), cdiv(N, GT), S), 256>>>(dH, dH, part, N, N, L);
        k_sum_parts<<<cdiv((long)N * N, 256), 256>>>(part, hht, (long)N * N, S);
        k_sweep<<<dim3(cdiv(P, 256), n_models), 256>>>(dmod, n_models, done, dW, P, N, 1, hht, N, xht, N, 1, vw);
        // H sweep: WtX = Wcat^T X [N][L] (entry t of column j at WtX[t][j]), WtW = Wcat^T Wcat
        k_gemm_tn<<<dim3(cdiv(L, GT), cdiv(N, GT)), 256>>>(dW, dX, wtx, N, L, P);
        k_gemm_tn<<<dim3(cdiv(N, GT), cdiv(N, GT)), 256>>>(dW, dW, wtw, N, N, P);
        k_sweep<<<dim3(cdiv(L, 256), n_models), 256>>>(dmod, n_models, done, dH, L, 1, L, wtw, N, wtx, 1, L, vh);
        k_finalize<<<n_models, RED>>>(done, dnit, vinit, trace, vw, P, vh, L, it, max_iter, tol);
        T_OK(hipGetLastError());
        if (it % POLL == 0 || it == max_iter) {
            T_OK(hipMemcpy(hdone.data(), done, n_models * sizeof(int), hipMemcpyDeviceToHost));
            if (std::all_of(hdone.begin(), hdone.end(), [](int d) { return d != 0; })) break;
        }
    }
    T_OK(hipEventRecord(e1, 0));
    T_OK(hipEventSynchronize(e1));
    float ms = 0.f;
    T_OK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (ms_per_iter) *ms_per_iter = ms / std::max(1, std::min(it, max_iter));

    // ||X - W H||_F and the sum of the relative residuals, per model
    const long nb = (long)cdiv(L, RED) * cdiv(P, ERR_ROWS);
    T_ALLOC(rpart.alloc((size_t)n_models * 2 * nb) || rout.alloc((size_t)n_models * 2));
    k_recon<<<(unsigned)nb, RED>>>(dmod, n_models, dX, dW, dH, P, L, N, rpart);
    k_recon_final<<<n_models, RED>>>(rpart, nb, rout);
    T_OK(hipGetLastError());

    std::vector<double> hout((size_t)n_models * 2);
    T_OK(hipMemcpy(hout.data(), rout, hout.size() * 8, hipMemcpyDeviceToHost));
    T_OK(hipMemcpy(n_iter, dnit, n_models * sizeof(int), hipMemcpyDeviceToHost));
    if (violation_trace && max_iter > 0)
        T_OK(hipMemcpy(violation_trace, trace, (size_t)n_models * max_iter * 8, hipMemcpyDeviceToHost));
    T_OK(hipMemcpy(wcat.data(), dW, (size_t)P * N * 4, hipMemcpyDeviceToHost));
    T_OK(hipMemcpy(H, dH, (size_t)N * L * 4, hipMemcpyDeviceToHost));
    for (int m = 0; m < n_models; ++m) {
        float *wm = W + (size_t)P * models[m].off;
        for (long i = 0; i < P; ++i)
            for (int k = 0; k < models[m].K; ++k) wm[(size_t)i * models[m].K + k] = wcat[(size_t)i * N + models[m].off + k];
        if (recon_err) recon_err[m] = hout[m * 2];
        if (mre) mre[m] = hout[m * 2 + 1] / ((double)P * (double)L);
    }
    return 0;
}

}  // extern "C"
