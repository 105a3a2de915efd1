// libhotmi355x — operator applications: block-ELL SpMV, restriction / prolongation, smoothers, V-cycle.
//
//   k_spmv          SquareMatrix::multiply (reference Projects/multigrid/SquareMatrix.h:477-487) — THE bandwidth consumer
//                   (SURVEY §8a row 17/21).  One wavefront per block row: a row is 125 contiguous 3x3 blocks (9000 B fp64),
//                   lane l owns slots l and l+64, so the 64 lanes stream the row in two fully coalesced sweeps; x is
//                   gathered per slot, the three row sums are reduced with __shfl_xor.
//   k_apmv_sub      the r -= A (P e) of the V-cycle as r -= (A P) e with the A P kept from the Galerkin build (half the bytes).
//   restrict/prolong SparseMPMMatrix::transposeMultiply / multiply on the transfer matrices (MPMMultigridMatrix.h:63-70) as
//                   pure gathers over the child / parent tables with scalar weights (the reference stores 3x3 w*I blocks).
//   smooth_dev      jacobi_smooth :160-173, optimal_jacobi_smooth :174-189, cg_smooth :190-226, chebyshev_smooth :227-264
//                   (+ SquareMatrix::estimate2norm), gs_smooth :266-318
//   vcycle_dev      MultigridOperator::operator() :362-421 with setup_parameters :525-551
#include "hot_impl.h"
#include "hot_svd.h"

namespace hot {

// ------------------------------------------------------------------------------------------------ vector ops
template <class T>
__global__ void k_axpy(size_t n, T a, const T* __restrict__ x, T* y)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += a * x[i];
}
template <class T>
__global__ void k_axpy_dev(size_t n, const double* a, double sign, const T* __restrict__ x, T* y)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    T s = (T)(sign * (*a));
    if (i < n) y[i] += s * x[i];
}
// y = x + (*a) * y
template <class T>
__global__ void k_xpay_dev(size_t n, const double* a, const T* __restrict__ x, T* y)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    T s = (T)(*a);
    if (i < n) y[i] = x[i] + s * y[i];
}
template <class T>
__global__ __launch_bounds__(256) void k_dot(size_t n, const T* __restrict__ x, const T* __restrict__ y, double* out, GridRed gr, const uint8_t* __restrict__ mask)
{
    __shared__ double red[4];
    double s = 0;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += 4 * stride) { // four strided elements per trip in flight
        T xv[4], yv[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t i = i0 + u * stride, ic = i < n ? i : i0;
            on[u] = i < n && (!mask || mask[ic / 3]); // sharded, halo mode: the rows this rank owns
            xv[u] = on[u] ? x[ic] : (T)0, yv[u] = on[u] ? y[ic] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (on[u]) s += (double)(xv[u] * yv[u]);
    }
    double t = block_sum_256<double>(s, red);
    grid_sum_store(t, 0.0, 1, gr, out, nullptr, red);
}
template <class T>
void Ctx<T>::axpy(size_t n, T a, const T* x, T* y)
{
    HOT_LAUNCH(this, "axpy", k_axpy<T>, div_up(n, 256), 256, 0, n, a, x, y);
}
template <class T>
void Ctx<T>::axpy_dev(size_t n, const double* a, double sign, const T* x, T* y)
{
    HOT_LAUNCH(this, "axpy", k_axpy_dev<T>, div_up(n, 256), 256, 0, n, a, sign, x, y);
}
// a plain kernel: a device-to-device hipMemcpyAsync between two kernels leaves the GPU idle for ~20 us on either side of the blit
template <class T>
__global__ __launch_bounds__(256) void k_copy(size_t n, const T* __restrict__ x, T* __restrict__ y)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = x[i];
}
// y := x, y2 := x (if not null), z := 0: the head of a V-cycle
template <class T>
__global__ __launch_bounds__(256) void k_vcycle_start(size_t n, const T* __restrict__ x, T* __restrict__ y, T* __restrict__ y2, T* __restrict__ z)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const T v = x[i];
        y[i] = v, z[i] = (T)0;
        if (y2) y2[i] = v;
    }
}
// ---- mixed precision: the fp64 vectors that enter and leave the fp32 V-cycle.
// y := x converted (round to nearest going down, exact going up): the vectors of hot_smooth / hot_restrict / hot_prolong / hot_spmv, exported fp32 data
template <class A, class B>
__global__ __launch_bounds__(256) void k_mg32_convert(size_t n, const A* __restrict__ x, B* __restrict__ y)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = (B)x[i];
}
// The largest magnitude of x and from it sc[0] = 2^-e, sc[1] = 2^e with 2^e <= max |x| < 2^(e+1) (e = 0 for an infinite maximum; fmax drops a NaN, so an x with NaN among finite entries is scaled by the finite maximum and the NaN goes through the V-cycle as it would in fp64; sc[1] = 0 marks an all-zero x; clamped to the
// exponents of normal numbers).  One launch, grid_sum_store's hand-off with a maximum in the place of the sum: every workgroup deposits its maximum, the
// one that arrives last takes the maximum of the deposits (exact in any order) and stores the scales; no floating-point atomics.  mirror: pinned host word
// that receives 2^e too (the absolute stopping test of a Jacobi top solver, smooth_dev kind 1, is applied to the unscaled residual).
__global__ __launch_bounds__(256) void k_mg32_absmax(size_t n, const double* __restrict__ x, GridRed gr, double* sc, double* mirror)
{
    __shared__ double red[4];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    auto block_max = [&](double m) {
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        if (lane == 0) red[w] = m;
        __syncthreads();
        const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        __syncthreads();
        return r;
    };
    double m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmax(m, fabs(x[i]));
    m = block_max(m);
    const unsigned nb = gridDim.x;
    if (threadIdx.x == 0) {
        __hip_atomic_store(gr.part + blockIdx.x, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev = __hip_atomic_fetch_add(gr.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == nb - 1u;
    }
    __syncthreads();
    if (!s_last) return; // workgroup-uniform
    double a = 0;
    for (unsigned i = threadIdx.x; i < nb; i += 256) a = fmax(a, __hip_atomic_load(gr.part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    a = block_max(a);
    if (threadIdx.x == 0) {
        int e = (a > 0.0 && a < (double)INFINITY) ? ilogb(a) : 0;
        e = e < -1022 ? -1022 : e;
        const double down = scalbn(1.0, -e), up = scalbn(1.0, e);
        sc[0] = down, sc[1] = a == 0.0 ? 0.0 : up; // (an all-zero input: the exit writes zeros whatever the fp32 solvers made of a zero residual, 0 / 0 in the PCG's step length)
        if (mirror) *mirror = up; // a plain store: the host reads it only after the ticket of a later kernel on this stream (smooth_dev's round trip), which orders it
        __hip_atomic_store(gr.count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// k_vcycle_start of the fp32 hierarchy fed from an fp64 vector: y := float(x 2^-e), y2 := the same (if not null), z := 0
__global__ __launch_bounds__(256) void k_mg32_enter(size_t n, const double* __restrict__ x, const double* __restrict__ sc, float* __restrict__ y, float* __restrict__ y2, float* __restrict__ z)
{
    const double down = sc[0];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = (float)(x[i] * down); // the product is exact (a power of two, no underflow above the smallest fp32 subnormal's range), one rounding
        y[i] = v, z[i] = 0.0f;
        if (y2) y2[i] = v;
    }
}
// out := double(z) 2^e (exact); zeros for an all-zero input
__global__ __launch_bounds__(256) void k_mg32_exit(size_t n, const float* __restrict__ z, const double* __restrict__ sc, double* __restrict__ out)
{
    const double up = sc[1]; // 0: the input was all zero
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = up == 0.0 ? 0.0 : (double)z[i] * up;
}
template <class T>
void Ctx<T>::widen_dev(size_t n, const float* x, double* y)
{
    if (n) HOT_LAUNCH(this, "mg32_convert", (k_mg32_convert<float, double>), (int)std::min<size_t>(div_up(n, 256), 4096), 256, 0, n, x, y);
}
template <class T>
void Ctx<T>::narrow_dev(size_t n, const double* x, float* y)
{
    if (n) HOT_LAUNCH(this, "mg32_convert", (k_mg32_convert<double, float>), (int)std::min<size_t>(div_up(n, 256), 4096), 256, 0, n, x, y);
}
// The preconditioner of an fp64 context on the fp32 hierarchy: one reduction launch for the scale, the shadow's V-cycle with k_mg32_enter as its head
// (in the place of k_vcycle_start), one launch that widens and scales back.  The exponent never leaves the device.
template <class T>
void Ctx<T>::vcycle_mixed(const T* in, T* out)
{
    if constexpr (sizeof(T) == 8) {
        const size_t n0 = 3 * (size_t)mg32->levels[0]->n;
        double* sc = dscal.p + 230;
        const int grid = std::min(div_up(n0, 1024), 256);
        HOT_LAUNCH(this, "mg32_enter", k_mg32_absmax, grid, 256, 0, n0, in, gred(grid), sc, hscal + 252);
        mg32->mg32_io[0].reserve(n0);
        float* out32 = mg32->mg32_io[0].p;
        mg32->vcycle_head = [this, in, sc, n0](float* y, float* y2, float* z) {
            HOT_LAUNCH(this, "mg32_enter", k_mg32_enter, (int)std::min<size_t>(div_up(n0, 256), 2048), 256, 0, n0, in, sc, y, y2, z);
        };
        struct Unhook {
            Ctx<float>* c;
            ~Unhook() { c->vcycle_head = nullptr; }
        } unhook{ mg32 };
        mg32->vcycle_dev(nullptr, out32);
        fold_shadow_stats();
        HOT_LAUNCH(this, "mg32_exit", k_mg32_exit, (int)std::min<size_t>(div_up(n0, 256), 2048), 256, 0, n0, out32, sc, out);
    }
}

template <class T>
void Ctx<T>::copy(size_t n, const T* x, T* y)
{
    if (n) HOT_LAUNCH(this, "copy", k_copy<T>, (int)std::min<size_t>(div_up(n, 256), 2048), 256, 0, n, x, y);
}
template <class T>
void Ctx<T>::zero(size_t n, T* y)
{
    HOT_HIP(hipMemsetAsync(y, 0, n * sizeof(T), stream));
}
template <class T>
void Ctx<T>::dot_to(size_t n, const T* x, const T* y, double* out, double* mirror)
{
    const int grid = std::min(div_up(n, 1024), 256);
    if (vmask) { // partitioned vectors: local sum over the owned rows, summed over the ranks, then (if asked for) handed to the host slot
        HOT_LAUNCH(this, "dot", k_dot<T>, grid, 256, 0, n, x, y, out, gred(grid), vmask);
        reduce_scalars(out, 1);
        if (mirror) HOT_HIP(hipMemcpyAsync(mirror, out, sizeof(double), hipMemcpyDeviceToHost, stream));
        return;
    }
    HOT_LAUNCH(this, "dot", k_dot<T>, grid, 256, 0, n, x, y, out, gred(grid, mirror), (const uint8_t*)nullptr); // <= 256 deposits, summed in index order
}
template <class T>
double Ctx<T>::dot_host(size_t n, const T* x, const T* y)
{
    const int grid = std::min(div_up(n, 1024), 256);
    HOT_LAUNCH(this, "dot", k_dot<T>, grid, 256, 0, n, x, y, dscal.p + 100, gred(grid, hscal + 100, true), vmask); // the summing workgroup also writes the pinned host slot
    wait_ticket();
    if (vmask) c_allreduce(hscal + 100, 1, HOT_COMM_F64, HOT_COMM_SUM, false); // partitioned vectors: the ranks' sums over their own rows
    return hscal[100];
}

// ------------------------------------------------------------------------------------------------ SpMV
template <class T>
__global__ __launch_bounds__(256) void k_spmv(const int32_t* __restrict__ col, const T* __restrict__ val, const T* __restrict__ x, T* __restrict__ y, int n, const uint8_t* __restrict__ own)
{
    const int lane = threadIdx.x & 63;
    const int row = xcd_block() * 4 + (threadIdx.x >> 6);
    if (row >= n || (own && !own[row])) return; // sharded: rows of other ranks (wave-uniform)
    const int32_t* c = col + (int64_t)row * 125;
    const T* v = val + (int64_t)row * 1125;
    T s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        int k = lane + 64 * r;
        if (k < 125) {
            int j = c[k];
            const T* b = v + k * 9;
            T x0 = x[3 * (int64_t)j], x1 = x[3 * (int64_t)j + 1], x2 = x[3 * (int64_t)j + 2];
            s0 += b[0] * x0 + b[3] * x1 + b[6] * x2;
            s1 += b[1] * x0 + b[4] * x1 + b[7] * x2;
            s2 += b[2] * x0 + b[5] * x1 + b[8] * x2;
        }
    }
    s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
    if (lane == 0) y[3 * (int64_t)row] = s0, y[3 * (int64_t)row + 1] = s1, y[3 * (int64_t)row + 2] = s2;
}
// r_i -= sum_J AP[i][J] e_J : the residual update after the coarse-grid correction.  A (P e) and (A P) e are the same
// vector; A P is a by-product of the Galerkin build with 64 window slots per row instead of the 125 of A, i.e. half
// the bytes of the SpMV the reference performs here (MultigridPreconditioner.h:362-421).
template <class T>
__global__ __launch_bounds__(256) void k_apmv_sub(const int32_t* __restrict__ apc, const T* __restrict__ apv, const T* __restrict__ e, T* __restrict__ r, int n, const uint8_t* __restrict__ own,
    T* unset /*not null: the level's GS forward target, marked "not written yet" here (see smooth_dev)*/)
{
    const int lane = threadIdx.x & 63;
    const int row = xcd_block() * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    if (unset && lane < 3) gs_store_unset(unset + 3 * (int64_t)row + lane);
    if (own && !own[row]) return;
    // lane = geometric window position; -1 where the window is structurally zero (an even coordinate's fourth coarse node): nothing is stored nor loaded
    // there, and the stored positions are packed in this order (k_ap): a lane's slot is its rank among the row's stored positions.  The wavefront sum
    // pairs the same positions as before the packing (the skipped ones used to add exact zeros): bit-identical results.
    const int j = nt_load(apc + (int64_t)row * 64 + lane);
    const int slot = __popcll(__ballot(j >= 0) & ((1ull << lane) - 1ull));
    T s0 = (T)0, s1 = (T)0, s2 = (T)0;
    if (j >= 0) {
        const T* bp = apv + ((int64_t)row * 64 + slot) * 9;
        T b[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) b[t] = nt_load(bp + t);
        const T x0 = e[3 * (int64_t)j], x1 = e[3 * (int64_t)j + 1], x2 = e[3 * (int64_t)j + 2];
        s0 = b[0] * x0 + b[3] * x1 + b[6] * x2;
        s1 = b[1] * x0 + b[4] * x1 + b[7] * x2;
        s2 = b[2] * x0 + b[5] * x1 + b[8] * x2;
    }
    s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
    if (lane == 0) r[3 * (int64_t)row] -= s0, r[3 * (int64_t)row + 1] -= s1, r[3 * (int64_t)row + 2] -= s2;
}
// ---- cg_smooth (MultigridPreconditioner.h:190-226) in three launches per iteration instead of nine.  Device scalars:
// s[0] z'r of the current iterate, s[1] du'A du, s[4] z'r of the next one, s[6] "s[4] is to become s[0]", s[7] z'r of the initial
// residual, s[8] the tolerance 0.25 s[7] (cgratio 0.5 squared, :203-209), s[9] iterations done.  The loop test `z'r < tol -> stop` is
// evaluated on the device: an iteration launched after convergence does nothing, so the host can enqueue a group of iterations and
// look at the outcome once (k_cg_direction leaves the latest z'r and the count in the pinned host slots `hm`).
__device__ __forceinline__ bool cg_active(double zTr, double tol) { return !(zTr < tol); }
template <class T>
__global__ void k_cg_setup(double* s, double* hm)
{
    const double tol = (double)(T)(s[7] * 0.25);
    s[8] = tol;
    s[1] = s[2] = s[3] = s[4] = s[5] = s[6] = s[9] = 0.0;
    hm[0] = s[0], hm[1] = 0.0, hm[2] = tol;
}
template <class T>
__global__ __launch_bounds__(256) void k_cg_spmv_dot(const int32_t* __restrict__ col, const T* __restrict__ val, const T* __restrict__ du, T* __restrict__ dAu, int n, double* s, GridRed gr)
{
    __shared__ double red[4];
    const bool roll = s[6] != 0.0;
    const double cur = roll ? s[4] : s[0]; // s[4] is not written in this launch; s[0] is read only where it is not
    if (blockIdx.x == 0 && threadIdx.x == 0 && roll) s[0] = s[4]; // also when converged: the two kernels that follow test s[0]
    if (!cg_active(cur, s[8])) return; // converged before this iteration
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    double part = 0;
    if (row < n) {
        const int32_t* c = col + (int64_t)row * 125;
        const T* v = val + (int64_t)row * 1125;
        T s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            int k = lane + 64 * r;
            if (k < 125) {
                int j = c[k];
                const T* b = v + k * 9;
                T x0 = du[3 * (int64_t)j], x1 = du[3 * (int64_t)j + 1], x2 = du[3 * (int64_t)j + 2];
                s0 += b[0] * x0 + b[3] * x1 + b[6] * x2;
                s1 += b[1] * x0 + b[4] * x1 + b[7] * x2;
                s2 += b[2] * x0 + b[5] * x1 + b[8] * x2;
            }
        }
        s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
        if (lane == 0) {
            dAu[3 * (int64_t)row] = s0, dAu[3 * (int64_t)row + 1] = s1, dAu[3 * (int64_t)row + 2] = s2;
            part = (double)(s0 * du[3 * (int64_t)row]) + (double)(s1 * du[3 * (int64_t)row + 1]) + (double)(s2 * du[3 * (int64_t)row + 2]);
        }
    }
    if (lane == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    const double t = threadIdx.x == 0 ? red[0] + red[1] + red[2] + red[3] : 0.0;
    __syncthreads();
    grid_sum_store(t, 0.0, 1, gr, s + 1, nullptr, red);
}
// u += w du ; r -= w A du ; z = Dinv r ; s[4] += z'r      (w = s[0] / s[1])
template <class T>
__global__ __launch_bounds__(256) void k_cg_update(const T* __restrict__ Dinv, const T* __restrict__ du, const T* __restrict__ dAu, T* __restrict__ u, T* __restrict__ r, T* __restrict__ z, int n, double* s, GridRed gr)
{
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (!cg_active(s[0], s[8])) return; // s[0] is the current z'r since k_cg_spmv_dot, and nothing writes it here
    const double omega = s[0] / s[1];
    const T wp = (T)omega, wm = (T)(-omega);
    double part = 0;
    if (i < n) {
        T rr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u[3 * (int64_t)i + c] += wp * du[3 * (int64_t)i + c];
            rr[c] = r[3 * (int64_t)i + c] + wm * dAu[3 * (int64_t)i + c];
            r[3 * (int64_t)i + c] = rr[c];
        }
        const T* d = Dinv + 9 * (int64_t)i;
        const T z0 = d[0] * rr[0] + d[3] * rr[1] + d[6] * rr[2], z1 = d[1] * rr[0] + d[4] * rr[1] + d[7] * rr[2], z2 = d[2] * rr[0] + d[5] * rr[1] + d[8] * rr[2];
        z[3 * (int64_t)i] = z0, z[3 * (int64_t)i + 1] = z1, z[3 * (int64_t)i + 2] = z2;
        part = (double)(z0 * rr[0]) + (double)(z1 * rr[1]) + (double)(z2 * rr[2]);
    }
    const double t = block_sum_256<double>(part, red);
    grid_sum_store(t, 0.0, 1, gr, s + 4, nullptr, red);
}
// du = z + b du      (b = s[4] / s[0])
template <class T>
__global__ void k_cg_direction(size_t n3, const T* __restrict__ z, T* __restrict__ du, double* s, double* hm, double* ticket, double ticket_val)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = cg_active(s[0], s[8]);
    if (act && i < n3) du[i] = z[i] + (T)(s[4] / s[0]) * du[i];
    if (i == 0) { // nobody reads s[6] / s[9] in this launch
        if (act) {
            s[6] = 1.0;
            const double cnt = s[9] + 1.0;
            s[9] = cnt;
            hm[0] = s[4], hm[1] = cnt;
        }
        if (ticket) host_ticket_store(ticket, ticket_val); // last launch of a group: the host is waiting for hm (Ctx::wait_ticket)
    }
}
// ---- cg_smooth on a SMALL top level as ONE persistent launch (C2 level 2: 5.4 k rows, a 49 MB matrix, ~6 iterations per V-cycle): the
// three launches per iteration above cost ~20 us each there, an iteration's arithmetic 10 us.  One workgroup per compute unit at most, rows
// dealt to wavefronts once and for all (a wavefront touches only its own rows of u, r, z, dAu: plain loads / stores); du is the one vector
// read across workgroups (the SpMV's gathers): published with write-through stores and read with agent-scope loads, like k_gs_sweep's
// unknowns.  Three grid barriers per iteration (arrival counter + spin, all workgroups are resident); a dot product = every workgroup
// deposits its partial sum before the barrier and adds ALL deposits in index order after it, so every workgroup holds the same bits and
// takes the same exit decision.  Same recurrences as k_cg_spmv_dot / k_cg_update / k_cg_direction; only the association of the dot
// products differs.  count / exitc are zero between launches (the last workgroup to leave resets them).
// RPW > 0 (round 6): a wavefront has at most RPW rows, and everything of them stays ON THE COMPUTE UNIT for the whole solve — the matrix row in registers
// (lane k holds entries k and k + 64: 18 scalars + 2 column ids a row), D^-1, u, r, z, du, dAu of the row in 24 scalars of LDS that lane 0 works on.  An
// iteration then goes to memory for the gathers of du in the product and the publication of the new du, nothing else (the streaming version walks six
// dependent round trips an iteration besides its three barriers: 176 us a solve at C2's level 2, 5.4 k rows, of which the barriers are the smaller part).
// Same arithmetic, bit-identical results.
// Register budget: 1024 threads are four wavefronts per SIMD, 128 registers a lane; RPW = 2 in fp64 spends 76 on the matrix rows.  The rows' vectors are
// wave-uniform: held in registers of all 64 lanes (as first written) they were 96 more, and 137 registers went to scratch memory and back every iteration.
// What is uniform is therefore kept out of the vector registers — the wavefront's index, the recurrences' scalars (wave_first), the rows' vectors (LDS) —
// and the kernel has no scratch (tests/test_kernel_resources.py).
template <class T, int RPW = 0>
__global__ __launch_bounds__(1024) void k_cg_persist(const int32_t* __restrict__ col, const T* __restrict__ val, const T* __restrict__ Dinv, const T* __restrict__ init, T* __restrict__ u,
    T* __restrict__ r, T* __restrict__ z, T* du, T* __restrict__ dAu, int n, int max_iters, unsigned phase0 /*barriers this context's persistent solves have passed so far, mod 4*/, double* dep /*[4][gridDim.x][SS]*/, int SS /*doubles between two workgroups' slots*/, double* hm, double* ticket, double ticket_val,
    int* err /*pinned host word (k_gs_sweep's): a barrier that does not complete — the workgroups are not all resident because something else holds the chip — sets it; the host redoes the solve with launches*/)
{
    __shared__ double red[32], sres[2];
    __shared__ int s_bail;
    // RPW > 0: what lane 0 of a wavefront keeps of its rows between the barriers — D^-1 and the five vectors (6 KB in fp64 beside the dynamic du)
    enum { CG_DI = 0, CG_U = 9, CG_R = 12, CG_Z = 15, CG_D = 18, CG_AD = 21 };
    __shared__ T cg_row[RPW > 0 ? 16 : 1][RPW > 0 ? RPW : 1][24];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6); // (the wavefront's index, hence its rows and their addresses, in scalar registers)
    const int G = gridDim.x, wg = blockIdx.x;
    unsigned phase = phase0;
    if (tid == 0) s_bail = 0;
    auto ldu = [&](int64_t j, int c) { return __hip_atomic_load(du + 3 * j + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto sdu = [&](int64_t j, int c, T v) { __hip_atomic_store(du + 3 * j + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // Grid barrier + two dot products in one: workgroup-wide fixed-order sum of the wavefronts' lane-0 values, deposit, wait until every workgroup's
    // deposit of this phase is there, ordered sum of all deposits -> (o0, o1) everywhere.  The deposits are their own arrival flags (round 6; rounds 4 - 5:
    // deposit, wait for it to be performed, two-level arrival counters, poll, then fetch the deposits: five dependent trips to the memory side, ~5 us a
    // barrier, three barriers an iteration): four rotating sets of slots, a slot holds a signalling-NaN pattern no sum can produce until its owner writes
    // the phase's sums (write-through stores, agent-scope loads: k_gs_sweep's hand-off); with the deposit of phase p a workgroup resets its slots of phase
    // p + 2 — everybody has left phase p - 2, the previous tenant of that set, before anybody deposits for p - 1.  Wavefront 0 polls and sums the first
    // value, wavefront 1 the second: a lane adds slots lane, lane + 64, .. in ascending order, then the fixed DPP tree: the same bits everywhere.
    auto all_sum = [&](double v0, double v1, double& o0, double& o1) -> bool {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // every thread's write-through stores of du have been performed before its workgroup deposits
        if (lane == 0) red[w] = v0, red[16 + w] = v1;
        __syncthreads();
        // (a workgroup's two sums share a line; the workgroups' lines are SS doubles apart, so that the 256 pollers' uncached loads spread over the memory
        // channels instead of queueing on the one or two that hold a packed 4 KB array)
        double* d = dep + (size_t)(phase & 3u) * G * SS;
        if (tid == 0) {
            double t0 = 0, t1 = 0;
            for (int k = 0; k < 16; ++k) t0 += red[k], t1 += red[16 + k];
            double* dn = dep + (size_t)((phase + 2u) & 3u) * G * SS + (size_t)wg * SS;
            __hip_atomic_store((unsigned long long*)dn, GsUnset<double>::bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store((unsigned long long*)(dn + 1), GsUnset<double>::bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(d + (size_t)wg * SS, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(d + (size_t)wg * SS + 1, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (w < 2) {
            const double* dv = d + w;
            double a = 0;
            int spins = 0, bail = 0;
            for (;;) {
                bool all = true;
                a = 0;
                for (int k = lane; k < G; k += 64) {
                    const double x = __hip_atomic_load(dv + (size_t)k * SS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    all = all && !GsUnset<double>::is(x);
                    a += x;
                }
                if (__all(all)) break;
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (1 << 21) || ((spins & 255) == 0 && *(volatile int*)err)) { // (wave-uniform)
                    *(volatile int*)err = 1;
                    bail = 1;
                    break;
                }
            }
            a = wave_sum(a);
            if (lane == 0) {
                sres[w] = a;
                if (bail) s_bail = 1;
            }
        }
        __syncthreads();
        if (s_bail) return false; // workgroup-uniform
        o0 = wave_first(sres[0]), o1 = wave_first(sres[1]); // (uniform, and known to be: the scalars of the recurrences stay out of the vector registers)
        ++phase;
        return true;
    };
    auto scale = [&](int64_t i, const T (&v)[3], T (&o)[3]) {
        const T* d = Dinv + 9 * i;
        o[0] = d[0] * v[0] + d[3] * v[1] + d[6] * v[2], o[1] = d[1] * v[0] + d[4] * v[1] + d[7] * v[2], o[2] = d[2] * v[0] + d[5] * v[1] + d[8] * v[2];
    };
    const int stride = 16 * G;
    if constexpr (RPW > 0) {
        // ---- the register-resident version.  Register budget: 1024 threads = four wavefronts per SIMD = 128 registers a lane, of which the matrix rows
        // take 2 x (18 scalars + a column id) = 76 in fp64.  A row's vectors and D^-1 are wave-uniform and lane 0's business only: they live in the
        // wavefront's own 24 scalars of LDS per row (cg_row: D^-1, u, r, z, du, dAu), not in a register of every lane
        int rowq[RPW];
        int32_t mc[RPW][2];
        T mv[RPW][2][9];
        double p0 = 0, p1 = 0;
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const int row = wg * 16 + w + q * stride;
            rowq[q] = row < n ? row : -1;
            const int64_t rc = row < n ? row : 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = min(lane + 64 * h, 124);
                mc[q][h] = col[rc * 125 + k];
#pragma unroll
                for (int e = 0; e < 9; ++e) mv[q][h][e] = (lane + 64 * h < 125) ? val[rc * 1125 + k * 9 + e] : (T)0;
            }
            if (lane == 0) {
                T* st = cg_row[w][q];
                T di[9], a[3], za[3], rr[3], zz[3];
#pragma unroll
                for (int e = 0; e < 9; ++e) di[e] = Dinv[9 * rc + e], st[CG_DI + e] = di[e];
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = init[3 * rc + c], rr[c] = r[3 * rc + c], st[CG_U + c] = u[3 * rc + c], st[CG_AD + c] = (T)0;
#pragma unroll
                for (int c = 0; c < 3; ++c) za[c] = di[c] * a[0] + di[3 + c] * a[1] + di[6 + c] * a[2], zz[c] = di[c] * rr[0] + di[3 + c] * rr[1] + di[6 + c] * rr[2];
                if (rowq[q] >= 0) {
                    p0 += (double)(za[0] * a[0]) + (double)(za[1] * a[1]) + (double)(za[2] * a[2]);
                    p1 += (double)(zz[0] * rr[0]) + (double)(zz[1] * rr[1]) + (double)(zz[2] * rr[2]);
                    for (int c = 0; c < 3; ++c) sdu(row, c, zz[c]);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) st[CG_R + c] = rr[c], st[CG_Z + c] = zz[c], st[CG_D + c] = zz[c];
            }
        }
        double zTr0, zTr;
        if (!all_sum(p0, p1, zTr0, zTr)) return;
        const double tol = (double)(T)(zTr0 * 0.25); // cgratio 0.5, squared (MultigridPreconditioner.h:203-209)
        // The product gathers du from LDS: behind the barrier that publishes it every workgroup copies the WHOLE vector (3 n scalars: 140 KB at C2's level 2)
        // with 16-byte uncached loads, coalesced — 33 MB an iteration over the chip.  The streaming version gathers du entry by entry with agent-scope loads,
        // which pass the L2 one 8-byte request at a time: 2 M of them an iteration (5.4 k rows x 125 entries x 3), ~50 us — that, not the barriers, was an
        // iteration's cost (measured: neither a cheaper barrier nor one barrier fewer moved it; cached gathers behind an agent-scope acquire fence, which
        // invalidates the XCD's L2 from every wavefront, cost 2.6 x more).
        extern __shared__ double cg_lds[]; // [3 n] du
        T* ldsdu = (T*)cg_lds;
        const int n3 = 3 * n;
        auto pull_du = [&]() {
            const int n16 = n3 >> 1; // 16-byte pieces
            for (int e0 = 0; e0 < n16; e0 += 4 * 1024) {
                double2 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned eb = 16u * (unsigned)min(e0 + k * 1024 + tid, n16 - 1); // (scalar base + 32-bit offset: one address register a load, not two)
                    asm volatile("global_load_dwordx4 %0, %1, %2 sc0 sc1" : "=v"(v[k]) : "v"(eb), "s"(du) : "memory");
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = e0 + k * 1024 + tid;
                    if (e < n16) ((double2*)ldsdu)[e] = v[k];
                }
            }
            if ((n3 & 1) && tid == 0) ldsdu[n3 - 1] = ldu(n - 1, 2);
            __syncthreads();
        };
        int cnt = 0;
#ifdef HOT_AB_KERNELS
        unsigned long long tk[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, t0_ = wall_clock64(); // A/B build, HOT_CG_DBG: 100 MHz clock of workgroup 0 between the phases, summed over the iterations
#define CG_TK(i) \
    do { \
        const unsigned long long t_ = wall_clock64(); \
        tk[i] += t_ - t0_, t0_ = t_; \
    } while (0)
#else
#define CG_TK(i)
#endif
        for (; cnt < max_iters && cg_active(zTr, tol); ++cnt) {
            pull_du();
            CG_TK(0);
            double pd = 0;
#pragma unroll
            for (int q = 0; q < RPW; ++q) {
                T s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (lane + 64 * h < 125) {
                        const int j = mc[q][h];
                        const T* b = mv[q][h];
                        const T x0 = ldsdu[3 * j], x1 = ldsdu[3 * j + 1], x2 = ldsdu[3 * j + 2];
                        s0 += b[0] * x0 + b[3] * x1 + b[6] * x2;
                        s1 += b[1] * x0 + b[4] * x1 + b[7] * x2;
                        s2 += b[2] * x0 + b[5] * x1 + b[8] * x2;
                    }
                }
                s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
                if (lane == 0) {
                    T* st = cg_row[w][q];
                    st[CG_AD] = s0, st[CG_AD + 1] = s1, st[CG_AD + 2] = s2;
                    if (rowq[q] >= 0) pd += (double)(s0 * st[CG_D]) + (double)(s1 * st[CG_D + 1]) + (double)(s2 * st[CG_D + 2]);
                }
            }
            CG_TK(1);
            double dAd, unused;
            if (!all_sum(pd, 0.0, dAd, unused)) return;
            CG_TK(2);
            const double omega = zTr / dAd;
            const T wp = (T)omega, wm = (T)(-omega);
            double pz = 0;
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < RPW; ++q) {
                    T* st = cg_row[w][q];
                    T rr[3], zz[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) st[CG_U + c] += wp * st[CG_D + c], rr[c] = st[CG_R + c] + wm * st[CG_AD + c];
#pragma unroll
                    for (int c = 0; c < 3; ++c) zz[c] = st[CG_DI + c] * rr[0] + st[CG_DI + 3 + c] * rr[1] + st[CG_DI + 6 + c] * rr[2];
                    if (rowq[q] >= 0) pz += (double)(zz[0] * rr[0]) + (double)(zz[1] * rr[1]) + (double)(zz[2] * rr[2]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) st[CG_R + c] = rr[c], st[CG_Z + c] = zz[c];
                }
            }
            CG_TK(3);
            double zTrNew;
            if (!all_sum(pz, 0.0, zTrNew, unused)) return;
            CG_TK(4);
            const T beta = (T)(zTrNew / zTr);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < RPW; ++q) {
                    T* st = cg_row[w][q];
                    T dd[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) dd[c] = st[CG_Z + c] + beta * st[CG_D + c], st[CG_D + c] = dd[c];
                    if (rowq[q] >= 0)
                        for (int c = 0; c < 3; ++c) sdu(rowq[q], c, dd[c]);
                }
            }
            zTr = zTrNew;
            CG_TK(5);
            if (!all_sum(0.0, 0.0, unused, unused)) return;
            CG_TK(6);
        }
#ifdef HOT_AB_KERNELS
        if (tid == 0 && wg == 0)
            for (int i = 0; i < 7; ++i) hm[8 + i] = (double)tk[i];
#endif
        // what the streaming version leaves in memory: u, r, z, dAu of the last iteration (du has been published)
#pragma unroll
        for (int q = 0; q < RPW; ++q)
            if (lane == 0 && rowq[q] >= 0) {
                const T* st = cg_row[w][q];
                for (int c = 0; c < 3; ++c) {
                    const int64_t e = 3 * (int64_t)rowq[q] + c;
                    u[e] = st[CG_U + c], r[e] = st[CG_R + c], z[e] = st[CG_Z + c], dAu[e] = st[CG_AD + c];
                }
            }
        if (tid == 0 && wg == 0) {
            hm[0] = zTr, hm[1] = (double)cnt, hm[2] = tol, hm[3] = (double)(phase & 3u); // (hm[3]: the barrier set the next launch starts with — the host keeps its own count)
            if (ticket) host_ticket_store(ticket, ticket_val);
        }
        return;
    }
    // ---- set-up: z'r of the reference residual (the tolerance) and of r; du = z = Dinv r
    double p0 = 0, p1 = 0;
    for (int row = wg * 16 + w; row < n; row += stride) {
        if (lane == 0) {
            T a[3] = { init[3 * (int64_t)row], init[3 * (int64_t)row + 1], init[3 * (int64_t)row + 2] }, za[3];
            scale(row, a, za);
            p0 += (double)(za[0] * a[0]) + (double)(za[1] * a[1]) + (double)(za[2] * a[2]);
            T b[3] = { r[3 * (int64_t)row], r[3 * (int64_t)row + 1], r[3 * (int64_t)row + 2] }, zb[3];
            scale(row, b, zb);
            for (int c = 0; c < 3; ++c) z[3 * (int64_t)row + c] = zb[c], sdu(row, c, zb[c]);
            p1 += (double)(zb[0] * b[0]) + (double)(zb[1] * b[1]) + (double)(zb[2] * b[2]);
        }
    }
    double zTr0, zTr;
    if (!all_sum(p0, p1, zTr0, zTr)) return;
    const double tol = (double)(T)(zTr0 * 0.25); // cgratio 0.5, squared (MultigridPreconditioner.h:203-209)
    int cnt = 0;
    for (; cnt < max_iters && cg_active(zTr, tol); ++cnt) {
        // dAu = A du on this workgroup's rows, du'dAu
        double pd = 0;
        for (int row = wg * 16 + w; row < n; row += stride) {
            const int32_t* c = col + (int64_t)row * 125;
            const T* v = val + (int64_t)row * 1125;
            T s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = lane + 64 * q;
                if (k < 125) {
                    const int64_t j = c[k];
                    const T* b = v + k * 9;
                    const T x0 = ldu(j, 0), x1 = ldu(j, 1), x2 = ldu(j, 2);
                    s0 += b[0] * x0 + b[3] * x1 + b[6] * x2;
                    s1 += b[1] * x0 + b[4] * x1 + b[7] * x2;
                    s2 += b[2] * x0 + b[5] * x1 + b[8] * x2;
                }
            }
            s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
            if (lane == 0) {
                dAu[3 * (int64_t)row] = s0, dAu[3 * (int64_t)row + 1] = s1, dAu[3 * (int64_t)row + 2] = s2;
                pd += (double)(s0 * ldu(row, 0)) + (double)(s1 * ldu(row, 1)) + (double)(s2 * ldu(row, 2));
            }
        }
        double dAd, unused;
        if (!all_sum(pd, 0.0, dAd, unused)) return;
        // u += w du ; r -= w A du ; z = Dinv r ; z'r
        const double omega = zTr / dAd;
        const T wp = (T)omega, wm = (T)(-omega);
        double pz = 0;
        for (int row = wg * 16 + w; row < n; row += stride) {
            if (lane == 0) {
                T rr[3], zz[3];
                for (int c = 0; c < 3; ++c) {
                    u[3 * (int64_t)row + c] += wp * ldu(row, c);
                    rr[c] = r[3 * (int64_t)row + c] + wm * dAu[3 * (int64_t)row + c];
                    r[3 * (int64_t)row + c] = rr[c];
                }
                scale(row, rr, zz);
                for (int c = 0; c < 3; ++c) z[3 * (int64_t)row + c] = zz[c];
                pz += (double)(zz[0] * rr[0]) + (double)(zz[1] * rr[1]) + (double)(zz[2] * rr[2]);
            }
        }
        double zTrNew;
        if (!all_sum(pz, 0.0, zTrNew, unused)) return;
        // du = z + b du, published before the next SpMV gathers it
        const T beta = (T)(zTrNew / zTr);
        for (int row = wg * 16 + w; row < n; row += stride)
            if (lane == 0)
                for (int c = 0; c < 3; ++c) sdu(row, c, z[3 * (int64_t)row + c] + beta * ldu(row, c));
        zTr = zTrNew;
        if (!all_sum(0.0, 0.0, unused, unused)) return;
    }
    if (tid == 0) {
        if (wg == 0) {
            hm[0] = zTr, hm[1] = (double)cnt, hm[2] = tol, hm[3] = (double)(phase & 3u);
            if (ticket) host_ticket_store(ticket, ticket_val);
        }
    }
}

template <class T>
__global__ void k_scal_v(size_t n, T a, T* x)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= a;
}
template <class T>
void Ctx<T>::scal(size_t n, T a, T* x)
{
    HOT_LAUNCH(this, "scal", k_scal_v<T>, div_up(n, 256), 256, 0, n, a, x);
}
template <class T>
void Ctx<T>::spmv_dev(Level<T>& L, const T* x, T* y)
{
    if (L.part && halo_mode()) halo_gather(L, const_cast<T*>(x)); // the entries of x the owned rows couple to
    HOT_LAUNCH(this, lname("spmv", L.id).c_str(), k_spmv<T>, xcd_grid(div_up(L.n, 4)), 256, 0, L.col.p, L.val.p, x, y, L.n, L.mask());
    if (!halo_mode()) exchange(L, y, -1); // first-generation sharding: every rank computed the rows it owns; all of y is needed by the replicated vector algebra
}

// ------------------------------------------------------------------------------------------------ transfers
template <class T>
__global__ void k_restrict(const int32_t* __restrict__ child, const T* __restrict__ fine, T* coarse, int nc, const uint8_t* __restrict__ coarse_own, const uint8_t* __restrict__ fine_own,
    T* unset /*not null: the coarse level's GS forward target, marked "not written yet" here (see smooth_dev)*/, T* zero_out = nullptr /*not null: a coarse-level vector cleared on the way (the V-cycle's coarse iterate, instead of a fill launch)*/)
{
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * nc) return;
    if (unset) gs_store_unset(unset + e);
    if (zero_out) zero_out[e] = (T)0;
    int I = e / 3, d = e - 3 * I;
    if (coarse_own && !coarse_own[I]) return; // sharded, both levels partitioned: the coarse rows this rank owns (their children are in the fine halo)
    // all 27 child ids first, then all 27 values (clamped index, dropped by the select): two rounds of independent loads instead of
    // 27 dependent pairs; the sum keeps the child order
    int ci[27];
#pragma unroll
    for (int q = 0; q < 27; ++q) ci[q] = child[I * 27 + q];
    T fv[27];
#pragma unroll
    for (int q = 0; q < 27; ++q) fv[q] = fine[3 * (int64_t)(ci[q] < 0 ? 0 : ci[q]) + d];
    T s = 0;
#pragma unroll
    for (int q = 0; q < 27; ++q) {
        const T w = ((q / 9 != 1) ? (T)0.5 : (T)1) * (((q / 3) % 3 != 1) ? (T)0.5 : (T)1) * ((q % 3 != 1) ? (T)0.5 : (T)1);
        s = (ci[q] < 0 || (fine_own && !fine_own[ci[q]])) ? s : s + w * fv[q]; // fine_own: partial sum over this rank's fine rows (replicated coarse level, all-reduced)
    }
    coarse[e] = s;
}
template <class T>
__global__ void k_prolong(const int32_t* __restrict__ pcol, const T* __restrict__ pw, const T* __restrict__ coarse, T* fine, int n, const uint8_t* __restrict__ own)
{
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * n) return;
    int i = e / 3, d = e - 3 * i;
    if (own && !own[i]) return;
    T s = 0;
    for (int l = 0; l < 8; ++l) s += pw[8 * (int64_t)i + l] * coarse[3 * (int64_t)pcol[8 * (int64_t)i + l] + d];
    fine[e] = s;
}
template <class T>
int Ctx<T>::smoother_kind(int level, bool top) const
{
    const bool baseline = cfg.useBaselineMultigrid != 0; // GS smoother, PCG on top (MultigridSimulation.inl:446-453)
    const int splitLevel = cfg.topDownMGS ? 1 : cfg.levelCnt - 1;
    return (level < splitLevel && !top) ? (baseline ? 5 : cfg.smoother) : (baseline ? 2 : cfg.coarseSolver);
}
// the level's next smoother is the chained GS sweep that takes its forward target's "not written yet" marks from the kernel before it
template <class T>
bool Ctx<T>::gs_marks_wanted(int level) const
{
    return smoother_kind(level) == 5 && gs_plan(*levels[level]).marks;
}
template <class T>
void Ctx<T>::restrict_dev(int level, const T* fine, T* coarse, T* zero_coarse)
{
    Level<T>& C = *levels[level + 1];
    Level<T>& F = *levels[level];
    if (F.part && halo_mode()) {
        if (zero_coarse) zero(3 * (size_t)C.n, zero_coarse);
        if (C.part) { // owner of a coarse row sums its 27 children: those owned elsewhere come with the fine level's halo
            halo_gather(F, const_cast<T*>(fine));
            HOT_LAUNCH(this, "restrict", k_restrict<T>, div_up(3 * (size_t)C.n, 256), 256, 0, C.child.p, fine, coarse, C.n, C.own.p, (const uint8_t*)nullptr, (T*)nullptr);
        }
        else { // replicated coarse level: every rank sums the children it owns, one all-reduce of the (small) coarse vector completes the rows
            HOT_LAUNCH(this, "restrict", k_restrict<T>, div_up(3 * (size_t)C.n, 256), 256, 0, C.child.p, fine, coarse, C.n, (const uint8_t*)nullptr, F.own.p, (T*)nullptr);
            CommTag tag(this, "coarse_vector_allreduce");
            c_allreduce(coarse, 3 * (int64_t)C.n, REAL, HOT_COMM_SUM, true);
        }
        return;
    }
    // (every smoother on the coarse level is preceded by a restriction into it: its GS forward target gets its marks here)
    T* mark = gs_marks_wanted(level + 1) ? C.tmp.p : (T*)nullptr;
    HOT_LAUNCH(this, "restrict", k_restrict<T>, div_up(3 * (size_t)C.n, 256), 256, 0, C.child.p, fine, coarse, C.n, (const uint8_t*)nullptr, (const uint8_t*)nullptr, mark, zero_coarse);
    unset_level = mark ? level + 1 : -1;
}
template <class T>
void Ctx<T>::prolong_dev(int level, const T* coarse, T* fine)
{
    Level<T>& F = *levels[level];
    Level<T>& C = *levels[level + 1];
    const bool hm = F.part && halo_mode();
    if (hm && C.part) halo_gather(C, const_cast<T*>(coarse)); // the parents / window columns of the fine rows this rank owns (also read by the k_apmv_sub that follows)
    HOT_LAUNCH(this, "prolong", k_prolong<T>, div_up(3 * (size_t)F.n, 256), 256, 0, F.pcol.p, F.pw.p, coarse, fine, F.n, hm ? F.own.p : (const uint8_t*)nullptr);
}

// ------------------------------------------------------------------------------------------------ smoothers
// mr_i = Dinv_i r_i (scale_diagonal_{entry,block}_inverse, MultigridPreconditioner.h:143-154)
template <class T>
__global__ void k_scale(const T* __restrict__ D, const T* __restrict__ r, T* mr, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T* d = D + 9 * (int64_t)i;
    T a = r[3 * (int64_t)i], b = r[3 * (int64_t)i + 1], c = r[3 * (int64_t)i + 2];
    mr[3 * (int64_t)i] = d[0] * a + d[3] * b + d[6] * c;
    mr[3 * (int64_t)i + 1] = d[1] * a + d[4] * b + d[7] * c;
    mr[3 * (int64_t)i + 2] = d[2] * a + d[5] * b + d[8] * c;
}

// SquareMatrix::estimate2norm (reference Projects/multigrid/SquareMatrix.h:375-475, active #else branch): power iteration on
// A*A from a +-1 start vector.  The reference seeds the signs with srand(time(NULL)); here they are a fixed hash of the
// entry index, the converged value does not depend on it within the 1e-6 stopping tolerance.
template <class T>
__global__ void k_cheb_start(T* v, size_t n3)
{
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n3) v[e] = ((((unsigned)e * 2654435761u) >> 16) & 1u) ? (T)1 : (T)-1;
}
template <class T>
__global__ void k_abs(T* v, size_t n3)
{
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n3) v[e] = v[e] < 0 ? -v[e] : v[e];
}
template <class T>
__global__ void k_div1(T* v, T c, size_t n3)
{
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n3) v[e] = v[e] / c;
}
template <class T>
void Ctx<T>::estimate_2norm(Level<T>& L, double tol)
{
    MaskScope mscope(this, halo_mode() ? L.mask() : nullptr); // this level's vectors (halo mode: the rows the rank owns)
    constexpr int MaxIters = 512;
    size_t n3 = 3 * (size_t)L.n;
    T *v = L.du.p, *x = L.dAu.p; // work vectors of the level, free while the hierarchy is being built
    HOT_LAUNCH(this, "cheb_start", k_cheb_start<T>, div_up(n3, 256), 256, 0, v, n3);
    spmv_dev(L, v, x);
    HOT_LAUNCH(this, "cheb_abs", k_abs<T>, div_up(n3, 256), 256, 0, x, n3);
    T e = (T)std::sqrt(dot_host(n3, x, x));
    if (e == 0) {
        L.lMin = L.lMax = 0;
        return;
    }
    HOT_LAUNCH(this, "cheb_div", k_div1<T>, div_up(n3, 256), 256, 0, x, e, n3);
    T e0 = 0;
    for (int iter = 0; iter < MaxIters && std::abs(e - e0) > (T)tol * e; ++iter) {
        e0 = e;
        spmv_dev(L, x, v);
        spmv_dev(L, v, x);
        T normx = (T)std::sqrt(dot_host(n3, x, x));
        e = normx / (T)std::sqrt(dot_host(n3, v, v));
        HOT_LAUNCH(this, "cheb_div", k_div1<T>, div_up(n3, 256), 256, 0, x, normx, n3);
    }
    L.lMax = e;
    L.lMin = L.lMax / 30; // "experience" (:473)
}

// out_i = D_i in_i for an arbitrary array of 3x3 blocks (matrix-free block-diagonal preconditioner)
template <class T>
void Ctx<T>::block_apply_dev(const T* D, const T* in, T* out, int n)
{
    HOT_LAUNCH(this, "diag_scale", k_scale<T>, div_up(n, 256), 256, 0, D, in, out, n);
}
template <class T>
void Ctx<T>::scale_dev(Level<T>& L, const T* in, T* out)
{
    HOT_LAUNCH(this, "diag_scale", k_scale<T>, div_up(L.n, 256), 256, 0, L.diagInv.p, in, out, L.n);
}

template <class T>
__global__ void k_cg_scalars(double* s, int what)
{
    // s[0]=zTrk  s[1]=dAu.du  s[2]=omega  s[3]=-omega  s[4]=zTrk_new  s[5]=beta
    if (what == 0) {
        s[2] = s[0] / s[1];
        s[3] = -s[2];
    }
    else {
        s[5] = s[4] / s[0];
        s[0] = s[4];
    }
}

// final_residual = false: the caller never reads r after this call (the post-smoothing leg of the V-cycle: the
// reference updates the residual there too, MultigridPreconditioner.h:266-318, but nothing consumes it), so the last
// residual update of the stationary smoothers is skipped.  The iterates u are unaffected.
template <class T>
void Ctx<T>::smooth_dev(int level, int kind, int iterations, T tolerance, T* u, T* r, T* du, T* dAu, bool final_residual)
{
    Level<T>& L = *levels[level];
    size_t n3 = 3 * (size_t)L.n;
    MaskScope mscope(this, halo_mode() ? L.mask() : nullptr); // halo mode: this level's vectors live on the rows the rank owns (replicated level: everywhere)
    const bool tmp_marked = unset_level == level; // L.tmp carries the chained GS sweep's "not written yet" marks (restrict_dev / vcycle_dev ran just before)
    unset_level = -1; // whatever this call does with L.tmp, the marks are spent
    auto Aproject = [&](T* v) {
        if (level == 0 && !cfg.systemBCProject) project_dev(v);
    };
    auto scaler = [&](const T* in, T* out) { scale_dev(L, in, out); };
    if (kind == 0) {
        for (; iterations--;) {
            scaler(r, du);
            scal(n3, (T)cfg.topomega, du);
            axpy(n3, (T)1, du, u);
            if (!final_residual && iterations == 0) break;
            spmv_dev(L, du, dAu);
            Aproject(dAu);
            axpy(n3, (T)-1, dAu, r);
        }
    }
    else if (kind == 1) {
        for (; iterations--;) {
            double rr = dot_host(n3, r, r);
            if (std::sqrt(rr) * (in_scale_h ? *in_scale_h : 1.0) < (double)tolerance) break; // (the shadow of a mixed-precision context: the test is on the unscaled residual)
            scaler(r, du);
            spmv_dev(L, du, dAu);
            Aproject(dAu);
            double a = dot_host(n3, du, r), b = dot_host(n3, du, dAu);
            T omega = (T)(a / b);
            axpy(n3, omega, du, u);
            axpy(n3, -omega, dAu, r);
        }
    }
    else if (kind == 2) {
        T* z = L.tmp.p;
        double* s = dscal.p + 40;
        const bool cg_unfused = ab_flag("HOT_CG_UNFUSED"); // A/B build only: one launch per vector operation
        const bool fused = !cg_unfused && !(level == 0 && !cfg.systemBCProject) && !L.part; // (partitioned level: the generic path below, whose SpMV exchanges)
        int cnt = 0;
        double zTrk = 0, tol = 0;
        // (not when ranks may share a device, nor after a spinning kernel has timed out on this context; fp64 only: in float the association of
        // the dot products decides which of several line-search halvings is taken two iterations later — cond ~ 1e8 —, and the whole-step fp32
        // parity test was validated against the launch-per-operation sums)
        if (fused && sizeof(T) == 8 && L.n <= 65536 && !gs_no_chain && !sharded() && !ab_flag("HOT_CG_LAUNCHES")) { // A/B build: HOT_CG_LAUNCHES = three launches per iteration on small levels too
            // the whole solve in one persistent launch (k_cg_persist), one host round trip for the iteration count
            const int G = std::min(std::min(ab_int("HOT_CG_WGS", 256), device_cus()), div_up(L.n, 16)); // 1024-thread workgroups that must all be resident: one per compute unit at most
            const int cg_ss = ab_int("HOT_CG_SLOT_STRIDE", 32); // doubles between the workgroups' deposit slots
            if (!cg_dep.p || cg_bar_dirty || cg_G != G) { // the deposit slots start "not written" (k_cg_persist's barrier); again after a launch that gave up — a barrier timed
                // out, which switches this path off until rearm_chain() switches it on 32 clean steps later — and when the grid changes (the slots are laid out by it)
                cg_dep.reserve((size_t)4 * 256 * cg_ss);
                HOT_LAUNCH(this, "gs_fill_unset", k_gs_fill_unset<double>, div_up((size_t)4 * 256 * cg_ss, 256), 256, 0, (size_t)4 * 256 * cg_ss, cg_dep.p);
                cg_bar_dirty = false, cg_G = G, cg_phase = 0;
            }
            // (levels of up to two rows per wavefront: everything of a row stays in registers between the barriers; A/B build: HOT_CG_STREAM = the streaming version)
            const bool cg_resident = L.n <= 2 * 16 * G && 3 * (size_t)L.n * sizeof(double) <= 150 * 1024 && !ab_flag("HOT_CG_STREAM"); // (du of the whole level in LDS)
            if (cg_resident && !attr_cg_set) {
                HOT_HIP(hipFuncSetAttribute((const void*)k_cg_persist<T, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
                attr_cg_set = true;
            }
            if (cg_resident)
                HOT_LAUNCH(this, lname("cg_persistent", L.id).c_str(), (k_cg_persist<T, 2>), G, 1024, 3 * (size_t)L.n * sizeof(double), L.col.p, L.val.p, L.diagInv.p, L.initialResidual.p, u, r, z, du, dAu, L.n, iterations, cg_phase, cg_dep.p, cg_ss,
                    hscal + 40, hscal + 251, new_ticket(), (int*)(hscal + 250));
            else
                HOT_LAUNCH(this, lname("cg_persistent", L.id).c_str(), k_cg_persist<T>, G, 1024, 0, L.col.p, L.val.p, L.diagInv.p, L.initialResidual.p, u, r, z, du, dAu, L.n, iterations, cg_phase, cg_dep.p, cg_ss,
                    hscal + 40, hscal + 251, new_ticket(), (int*)(hscal + 250));
            wait_ticket(); // a timed-out barrier shows in hscal[250]: sync() inside throws ERR_RETRY and the caller redoes the operation with launches
            cnt = (int)hscal[41];
            if (ab_flag("HOT_CG_DBG")) // A/B build: 10 ns ticks of workgroup 0 by phase
                fprintf(stderr, "cg_persistent level %d: %d rows, %d workgroups, %d iterations; ticks pull %.0f product %.0f barrier1 %.0f update %.0f barrier2 %.0f direction %.0f barrier3 %.0f\n", L.id, L.n, G, cnt,
                    hscal[48], hscal[49], hscal[50], hscal[51], hscal[52], hscal[53], hscal[54]);
            cg_phase = (cg_phase + 1u + 3u * (unsigned)cnt) & 3u; // one barrier at the set-up, three an iteration
            HOT_CHECK((unsigned)hscal[43] == cg_phase, HOT_ERR_DEVICE, "k_cg_persist passed another number of barriers than the host counts: the next launch would start on the wrong set of deposit slots");
            iterations = 0;
        }
        else if (fused) {
            // no host round trip before the first iteration and one per group of iterations afterwards (see k_cg_setup)
            scaler(L.initialResidual.p, z);
            dot_to(n3, z, L.initialResidual.p, s + 7);
            scaler(r, z);
            copy(n3, z, du);
            dot_to(n3, z, r, s);
            HOT_LAUNCH(this, "cg_setup", k_cg_setup<T>, 1, 1, 0, s, hscal + 40);
            int group = std::max(1, std::min(cg_group, 16)); // as many iterations as the previous solve on this level needed
            bool active = true;
            while (iterations > 0 && active) {
                const int g = std::min(group, iterations);
                for (int k = 0; k < g; ++k) {
                    HOT_LAUNCH(this, lname("spmv", L.id).c_str(), k_cg_spmv_dot<T>, div_up(L.n, 4), 256, 0, L.col.p, L.val.p, du, dAu, L.n, s, gred(div_up(L.n, 4)));
                    HOT_LAUNCH(this, "cg_update", k_cg_update<T>, div_up(L.n, 256), 256, 0, L.diagInv.p, du, dAu, u, r, z, L.n, s, gred(div_up(L.n, 256)));
                    const bool last = k + 1 == g;
                    HOT_LAUNCH(this, "cg_direction", k_cg_direction<T>, div_up(n3, 256), 256, 0, n3, z, du, s, hscal + 40, last ? hscal + 251 : (double*)nullptr, last ? new_ticket() : 0.0);
                }
                iterations -= g;
                wait_ticket();
                active = !(hscal[40] < hscal[42]);
                group = 2;
            }
            cnt = (int)hscal[41];
            cg_group = cnt;
            iterations = 0;
        }
        else {
            scaler(L.initialResidual.p, z);
            double zTrk0 = dot_host(n3, z, L.initialResidual.p);
            scaler(r, z);
            copy(n3, z, du);
            zTrk = dot_host(n3, z, r);
            tol = (double)(T)(zTrk0 * 0.25); // cgratio = 0.5 hard-wired (:203-209)
            HOT_HIP(hipMemcpyAsync(s, &zTrk, sizeof(double), hipMemcpyHostToDevice, stream));
        }
        for (; iterations-- > 0;) {
            if (zTrk < tol) break;
            spmv_dev(L, du, dAu);
            Aproject(dAu);
            dot_to(n3, dAu, du, s + 1);
            HOT_LAUNCH(this, "cg_scalars", k_cg_scalars<T>, 1, 1, 0, s, 0);
            axpy_dev(n3, s + 2, 1.0, du, u);
            axpy_dev(n3, s + 3, 1.0, dAu, r);
            scaler(r, z);
            dot_to(n3, z, r, s + 4);
            HOT_LAUNCH(this, "cg_scalars", k_cg_scalars<T>, 1, 1, 0, s, 1);
            HOT_LAUNCH(this, "xpay", k_xpay_dev<T>, div_up(n3, 256), 256, 0, n3, s + 5, z, du);
            HOT_HIP(hipMemcpyAsync(hscal + 40, s, sizeof(double), hipMemcpyDeviceToHost, stream));
            sync();
            zTrk = hscal[40];
            ++cnt;
        }
        stats.linear_iterations += cnt;
    }
    else if (kind == 6) {
        // chebyshev_smooth (MultigridPreconditioner.h:227-264); the tolerance argument is unused there
        T* p = L.tmp.p;
        T d = (T)((L.lMax + L.lMin) / 2), c = (T)((L.lMax - L.lMin) / 2);
        int cnt = 1;
        iterations--;
        scaler(r, p);
        T alpha = 1 / d, beta;
        copy(n3, p, du);
        spmv_dev(L, du, dAu);
        Aproject(dAu);
        axpy(n3, alpha, du, u);
        axpy(n3, -alpha, dAu, r);
        for (; iterations-- > 0; ++cnt) {
            scaler(r, p);
            beta = (T)0.5 * c * c * alpha * alpha;
            if (cnt > 1) beta *= (T)0.5;
            alpha = 1 / (d - beta / alpha);
            scal(n3, beta, du); // du = p + beta du
            axpy(n3, (T)1, p, du);
            spmv_dev(L, du, dAu);
            Aproject(dAu);
            axpy(n3, alpha, du, u);
            if (!final_residual && iterations <= 0) break;
            axpy(n3, -alpha, dAu, r);
        }
    }
    else if (kind == 7)
        ic_smooth_dev(L, u, r, dAu);
    else if (kind == 5)
        gs_smooth_dev(level, iterations, u, r, du, dAu, final_residual, tmp_marked);
    else
        HOT_CHECK(false, HOT_ERR_INVALID, "unsupported smoother kind");
}

template <class T>
void Ctx<T>::vcycle_dev(const T* in, T* out)
{
    if (mixed()) { // mixed precision: every V-cycle of this context (L-BFGS's initial Hessian, the Newton solvers' M^-1, hot_vcycle) runs on the fp32 hierarchy
        vcycle_mixed(in, out);
        return;
    }
    int levelCnt = (int)levels.size();
    int times = cfg.times, levelscale = cfg.levelscale;
    int splitLevel;
    auto downIter = [&](int level) { return times + level * levelscale; };
    auto upIter = [&](int level) { return cfg.topDownMGS ? 0 : times + level * levelscale; };
    const bool baseline = cfg.useBaselineMultigrid != 0; // GS smoother, PCG on top, 10000 top iterations (MultigridSimulation.inl:446-453)
    auto topIter = [&](int level) {
        if (cfg.topDownMGS || baseline) return 10000;
        if (cfg.levelCnt == 1) return times + level * levelscale;
        if (!(cfg.coarseSolver == 2 || cfg.coarseSolver == 6)) return (times + level * levelscale) * 3;
        return 10000;
    };
    splitLevel = cfg.topDownMGS ? 1 : cfg.levelCnt - 1;
    T tolTop = (T)(cfg.cneps * cfg.cneps);
    auto run = [&](bool regular, int level, T* sol, int its, bool final_residual = true) {
        Level<T>& L = *levels[level];
        smooth_dev(level, smoother_kind(level, !regular), its, regular ? (T)0 : tolTop, sol, L.residual.p, L.du.p, L.dAu.p, final_residual);
    };
    stats.vcycles++;
    Level<T>& L0 = *levels[0];
    size_t n0 = 3 * (size_t)L0.n;
    // residual := in (dRhs == 0, ImplicitSolver.h:483-484,579: correctResidualProjection is the identity), out := 0 and, on a single level, the
    // top solver's initial residual: one launch instead of two copies and a fill
    if (vcycle_head) // the shadow of a mixed-precision context: its parent's fp64 vector, scaled and rounded (k_mg32_enter)
        vcycle_head(L0.residual.p, levelCnt > 1 ? (T*)nullptr : L0.initialResidual.p, out);
    else
    HOT_LAUNCH(this, "vcycle_start", k_vcycle_start<T>, (int)std::min<size_t>(div_up(n0, 256), 2048), 256, 0, n0, in, L0.residual.p, levelCnt > 1 ? (T*)nullptr : L0.initialResidual.p, out);

    if (levelCnt > 1) restrict_dev(0, L0.residual.p, levels[1]->initialResidual.p);
    for (int l = 1; l < levelCnt - 1; ++l) restrict_dev(l, levels[l]->initialResidual.p, levels[l + 1]->initialResidual.p);
    int level;
    for (level = 0; level < levelCnt - 1; ++level) {
        T* sol = level == 0 ? out : levels[level]->sol.p;
        run(level < splitLevel, level, sol, level < splitLevel ? upIter(level) : topIter(level));
        restrict_dev(level, levels[level]->residual.p, levels[level + 1]->residual.p, levels[level + 1]->sol.p); // (clears the coarse iterate on the way)
    }
    run(false, level, level == 0 ? out : levels[level]->sol.p, topIter(level));
    for (--level; level >= 0; --level) {
        Level<T>& L = *levels[level];
        T* sol = level == 0 ? out : L.sol.p;
        size_t n3 = 3 * (size_t)L.n;
        prolong_dev(level, levels[level + 1]->sol.p, L.du.p);
        axpy(n3, (T)1, L.du.p, sol);
        const bool full_spmv = ab_flag("HOT_MG_FULL_SPMV"); // A/B build only: r -= A (P e) like the reference
        if (full_spmv) {
            spmv_dev(L, L.du.p, L.dAu.p);
            axpy(n3, (T)-1, L.dAu.p, L.residual.p);
        }
        else
        {
            T* mark = gs_marks_wanted(level) ? L.tmp.p : (T*)nullptr;
            HOT_LAUNCH(this, lname("apmv", L.id).c_str(), k_apmv_sub<T>, xcd_grid(div_up(L.n, 4)), 256, 0, L.apc.p, L.apv.p, levels[level + 1]->sol.p, L.residual.p, L.n, L.mask(), mark);
            unset_level = mark ? level : -1;
        }
        if (L.part && !halo_mode() && smoother_kind(level) != 5)
            exchange(L, L.residual.p, -1); // a GS post-smoother reads only the rows it owns; every other smoother runs replicated vector algebra on all of r
        run(level < splitLevel, level, sol, level < splitLevel ? downIter(level) : topIter(level), false);
    }
}

template <class T>
void Ctx<T>::precondition_dev(const T* in, T* out)
{
    HOT_CHECK(mixed() || (!levels.empty() && levels[0]->built), HOT_ERR_INVALID, "preconditioner used before hot_build_mg");
    vcycle_dev(in, out);
}

// ------------------------------------------------------------------------------------------------ C ABI wrappers
template <class T>
void Ctx<T>::spmv(int32_t level, const void* x, void* y)
{
    if constexpr (sizeof(T) == 8)
        if (mixed() && level >= 1) { // mixed precision: levels >= 1 exist only in fp32 (level 0 stays the fp64 Hessian: the operator of the Newton solvers)
            need(level < nlevels(), "level out of range");
            Level<float>& S = *mg32->levels[level];
            mixed_apply(x, 3 * (size_t)S.n, y, 3 * (size_t)S.n, [&](float* a, float* b) { mg32->spmv_dev(S, a, b); });
            return;
        }
    need(level >= 0 && level < (int)levels.size(), "level out of range");
    Level<T>& L = *levels[level];
    size_t n3 = 3 * (size_t)L.n;
    DBuf<T> a, b;
    a.reserve(n3), b.reserve(n3);
    HOT_HIP(hipMemcpyAsync(a.p, x, n3 * sizeof(T), hipMemcpyDefault, stream));
    spmv_dev(L, a.p, b.p);
    if (halo_mode()) gather_all(L, b.p); // the C ABI hands out complete vectors
    download(y, b.p, n3);
    sync();
}
template <class T>
void Ctx<T>::restrict_(int32_t level, const void* fine, void* coarse)
{
    if constexpr (sizeof(T) == 8)
        if (mixed()) {
            need(level >= 0 && level + 1 < nlevels(), "level out of range");
            mixed_apply(fine, 3 * (size_t)mg32->levels[level]->n, coarse, 3 * (size_t)mg32->levels[level + 1]->n, [&](float* a, float* b) { mg32->restrict_dev(level, a, b), mg32->unset_level = -1; });
            return;
        }
    need(level >= 0 && level + 1 < (int)levels.size(), "level out of range");
    size_t nf = 3 * (size_t)levels[level]->n, nc = 3 * (size_t)levels[level + 1]->n;
    DBuf<T> a, b;
    a.reserve(nf), b.reserve(nc);
    HOT_HIP(hipMemcpyAsync(a.p, fine, nf * sizeof(T), hipMemcpyDefault, stream));
    restrict_dev(level, a.p, b.p);
    if (halo_mode()) gather_all(*levels[level + 1], b.p);
    download(coarse, b.p, nc);
    sync();
}
template <class T>
void Ctx<T>::prolong(int32_t level, const void* coarse, void* fine)
{
    if constexpr (sizeof(T) == 8)
        if (mixed()) {
            need(level >= 0 && level + 1 < nlevels(), "level out of range");
            mixed_apply(coarse, 3 * (size_t)mg32->levels[level + 1]->n, fine, 3 * (size_t)mg32->levels[level]->n, [&](float* a, float* b) { mg32->prolong_dev(level, a, b); });
            return;
        }
    need(level >= 0 && level + 1 < (int)levels.size(), "level out of range");
    size_t nf = 3 * (size_t)levels[level]->n, nc = 3 * (size_t)levels[level + 1]->n;
    DBuf<T> a, b;
    a.reserve(nc), b.reserve(nf);
    HOT_HIP(hipMemcpyAsync(a.p, coarse, nc * sizeof(T), hipMemcpyDefault, stream));
    prolong_dev(level, a.p, b.p);
    if (halo_mode()) gather_all(*levels[level], b.p);
    download(fine, b.p, nf);
    sync();
}
template <class T>
void Ctx<T>::smooth(int32_t level, int32_t kind, int32_t iterations, double tol, void* u, void* r, const void* r0)
{
    if constexpr (sizeof(T) == 8)
        if (mixed()) { // the fp32 operators on every level, level 0 included; u, r, r0 rounded to nearest on the way in, widened on the way out
            need(level >= 0 && level < nlevels() && mg32->levels[level]->built, "hot_smooth: level not built (hot_build_mg)");
            Level<float>& S = *mg32->levels[level];
            const size_t n3 = 3 * (size_t)S.n;
            DBuf<T> keep[3];
            for (auto& k : keep) k.reserve(n3);
            HOT_HIP(hipMemcpyAsync(keep[0].p, u, n3 * sizeof(T), hipMemcpyDefault, stream));
            HOT_HIP(hipMemcpyAsync(keep[1].p, r, n3 * sizeof(T), hipMemcpyDefault, stream));
            HOT_HIP(hipMemcpyAsync(keep[2].p, r0 ? r0 : r, n3 * sizeof(T), hipMemcpyDefault, stream));
            for (auto& b : mg32->mg32_io) b.reserve(n3);
            hscal[252] = 1.0; // nothing was scaled: absolute stopping tests as they stand
            with_gs_retry([&] {
                narrow_dev(n3, keep[0].p, mg32->mg32_io[0].p), narrow_dev(n3, keep[1].p, mg32->mg32_io[1].p), narrow_dev(n3, keep[2].p, S.initialResidual.p);
                mg32->smooth_dev(level, kind, iterations, (float)tol, mg32->mg32_io[0].p, mg32->mg32_io[1].p, S.du.p, S.dAu.p);
                fold_shadow_stats();
                sync();
            });
            widen_dev(n3, mg32->mg32_io[0].p, keep[0].p), widen_dev(n3, mg32->mg32_io[1].p, keep[1].p);
            download(u, keep[0].p, n3);
            download(r, keep[1].p, n3);
            sync();
            return;
        }
    need(level >= 0 && level < (int)levels.size() && levels[level]->built, "hot_smooth: level not built (hot_build_mg)");
    Level<T>& L = *levels[level];
    size_t n3 = 3 * (size_t)L.n;
    DBuf<T> du_, dr_, r0_;
    du_.reserve(n3), dr_.reserve(n3), r0_.reserve(n3);
    HOT_HIP(hipMemcpyAsync(r0_.p, r0 ? r0 : r, n3 * sizeof(T), hipMemcpyDefault, stream)); // r may be overwritten below
    with_gs_retry([&] {
        HOT_HIP(hipMemcpyAsync(du_.p, u, n3 * sizeof(T), hipMemcpyDefault, stream));
        HOT_HIP(hipMemcpyAsync(dr_.p, r, n3 * sizeof(T), hipMemcpyDefault, stream));
        HOT_HIP(hipMemcpyAsync(L.initialResidual.p, r0_.p, n3 * sizeof(T), hipMemcpyDeviceToDevice, stream));
        smooth_dev(level, kind, iterations, (T)tol, du_.p, dr_.p, L.du.p, L.dAu.p);
        if (halo_mode()) gather_all(L, du_.p), gather_all(L, dr_.p);
        sync();
    });
    download(u, du_.p, n3);
    download(r, dr_.p, n3);
    sync();
}
template <class T>
void Ctx<T>::vcycle(const void* in, void* out)
{
    need(mixed() || (!levels.empty() && levels[0]->built), "hot_vcycle before hot_build_mg");
    size_t n3 = 3 * (size_t)Nn;
    HOT_HIP(hipMemcpyAsync(work0.p, in, n3 * sizeof(T), hipMemcpyDefault, stream));
    with_gs_retry([&] {
        vcycle_dev(work0.p, work1.p);
        if (halo_mode()) gather_all(*levels[0], work1.p);
        sync();
    });
    download(out, work1.p, n3);
    sync();
}

template struct Ctx<float>;
template struct Ctx<double>;

} // namespace hot
