// Per-(sample point, Gaussian) arithmetic shared by every kernel of the sampler.
//
// Semantics follow the reference's dense PyTorch twin of its CUDA sampler:
//   order 0  gaussians.sample_gaussians      /root/reference/gaussians.py:48-58
//   order 1  gaussians.gaussian_derivative   /root/reference/gaussians.py:89-101
//   order 2  gaussians.gaussian_derivative2  /root/reference/gaussians.py:103-116 (full Hessian)
//   order 3  its derivative wrt the sample point (shape n,d,d,d,c: model_pn.py:654)
// with  x = s - mu,  p = C x,  q = x.p,  g = exp(-q/2),  w_c = v_c g.
//
// Derivative outputs are symmetric in their derivative indices, so accumulators keep only the
// distinct components (D=2: xx,xy,yy and xxx,xxy,xyy,yyy) and expand on store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace pigs {

constexpr int ORD0 = 1, ORD1 = 2, ORD2 = 4, ORD3 = 8;
// trace of the Hessian (the Laplacian the PDE residuals consume, model_pn.py:614-617) instead of
// the full Hessian: one value per channel in the order-2 slot; never together with ORD2
constexpr int ORD2T = 16;
// A LINEAR RESIDUAL of the sampled field as the only output (mask == ORDR, alone):
//   r[m][c] = a0 u + a1 . grad u + aL (u_xx + u_yy) - target[m][c]
// -- the diffusion residual of the reference's losses (model_pn.py:612-617, 834-849;
// test_no_mlp.py:127-144: u_t - D lap u with u_t = (u - u_prev) / dt; the wave system mixes its channels: ORDC) in one launch and 4 B per point and
// channel instead of u, grad u and the Hessian (28 B).  Its backward is the backward of orders 0, 1 and
// the trace with the incoming gradients a0 gr, a1 gr, aL gr formed on the fly.
constexpr int ORDR = 32;
constexpr int ORDR_AS = ORD0 | ORD1 | ORD2T;      // the order mask whose backward arithmetic a residual uses

template <typename T> struct Resid {
    T a0, a1[2], aL;
    const T* target;      // [M][c] or null
};

// THE GENERAL RESIDUAL (mask == ORDG, alone): per-point coefficients and an advection term,
//   w_i(m)   = sum_c' B[i][c'] u_c'(x_m)
//   r[m][ch] = a0_m u_ch + sum_i a1_{m,i} d_i u_ch + aL_m lap u_ch + adv_m sum_i w_i(m) d_i u_ch - target[m][ch]
// -- the reference's time-blended losses (model_pn.py:794-805, IntegrationRule.TRAPEZOID; test_no_mlp.py:122-144,
// time_samples) and its Burgers term u u_x.  The product of two sums over the Gaussians is no sum over pairs, so the
// accumulators are those of orders 0, 1 and the trace (ORDR_AS) and the residual is composed once per point, where
// the finished sums are stored (fwd_store).  Its backward is the ORDR_AS backward with
//   g0[c'] = a0 gr_c' + adv sum_i B[i][c'] sum_ch gr_ch d_i u_ch,  g1[i][ch] = (a1_i + adv w_i) gr_ch,  trace = aL gr
// formed from gr, the coefficients and the forward's aux[m][1+d][c] = (u, d_i u)  (Gsym::load_terms).
constexpr int ORDG = 64;
// THE VORTICITY TERMS of a two-channel field u = (u_x, u_y) in two dimensions (mask == ORDV, alone; D == 2, C == 2):
// the seven numbers per point the reference's Navier-Stokes loss keeps of orders 0..3 (model_pn.py:650-659, 770-781,
// 848: div = ux[:,0,0] + ux[:,1,1], w = ux[:,0,1] - ux[:,1,0], wx = uxx[...,0,1] - uxx[...,1,0],
// lap w = trace of uxxx[...,0,1] - uxxx[...,1,0]) as one packed row
//   out[m][0..6] = (u_x, u_y, div u, w, w_x, w_y, lap w)
// Every one of them is a sum over the pairs, so the accumulators ARE the outputs: 7 slots instead of the 30 of
// orders 0..3 and 28 B per point instead of 120.  Its backward is the backward of orders 0..3 with the four
// incoming gradients formed on the fly from gout[m][0..6] (Gsym::load_vorticity).
constexpr int ORDV = 128;
constexpr int ORDV_AS = ORD0 | ORD1 | ORD2 | ORD3;
constexpr int NVORT = 7;
// THE COUPLED RESIDUAL (mask == ORDC, alone): the channels mixed by two constant c x c matrices under a per-point weight,
//   r[m][ch] = a0_m u_ch + aL_m lap u_ch + cw_m sum_c' (Q0[ch][c'] u_c' + QL[ch][c'] lap u_c') - target[m][ch]
// -- the reference's wave system (test_no_mlp.py:127-139, model_pn.py:623-627, 843-845: res0 = u_t[0] - ub[1],
// res1 = u_t[1] - (10 lap ub[0] - 0.1 ub[1]) with ub blended per point).  Nothing of grad u is read, so the accumulators
// are those of order 0 and the trace alone (ORDC_AS: 2 c of them, against the 2 c + d c of ORDG) and the residual is
// composed once per point in fwd_store.  Its backward is the ORDC_AS backward with
//   g0[c'] = a0 gr_c' + cw sum_ch Q0[ch][c'] gr_ch,  trace[c'] = aL gr_c' + cw sum_ch QL[ch][c'] gr_ch
// (Gsym::load_coupled): linear in the field, so no record of the forward is needed.
constexpr int ORDC = 256;
constexpr int ORDC_AS = ORD0 | ORD2T;
// THE VORTICITY RESIDUAL (mask == ORDN, alone; D == 2, C == 2): the Navier-Stokes residual in the vorticity formulation,
// composed from the seven sums of ORDV, a per-point time weight tau and the previous time level's seven prev[m][0..6]
// (null: zeros), with X_b = tau X + (1 - tau) X_prev for X in u_x, u_y, div, w_x, w_y, lap w:
//   out[m][0] = div_b
//   out[m][1] = time_term (w - w_prev) - dt (nu lap w_b - (u_x_b w_x_b + u_y_b w_y_b))
// -- compute_loss of the reference's model for Problem.NAVIER_STOKES under its three integration rules
// (model_pn.py:794-818, 629-631, 830, 848-849: tau per point = TRAPEZOID, 1 = BACKWARD, 0 = FORWARD).  The advection
// u . grad w is a product of two sums, so the accumulators are those of ORDV and the two numbers are composed once per
// point in fwd_store, which also leaves aux[m][0..3] = (u_x_b, u_y_b, w_x_b, w_y_b).  Its backward is the ORDV_AS
// backward with the seven incoming gradients formed from gout[m][0..1], the coefficients and that record
// (Gsym::load_vorticity_residual); prev is not read there.
constexpr int ORDN = 512;
// THE VORTICITY FIT (mask == ORDF, alone; D == 2, C == 2): the vorticity residual with the data term of the reference's
// Navier-Stokes loop and of its initialisation fit (main_pn.py:202-212, test_initialize.py:131-136) as a third column,
//   out[m][0..1] as for ORDN,   out[m][2] = data_weight (w - data[m])         (w of the CURRENT level, not blended)
// from the same seven sums; data [M] is a constant.  Its backward is that of ORDN with the gradient that arrives at w
// g_r time_term + g_f data_weight (Gsym::load_vorticity_fit); neither prev nor data is read there.
constexpr int ORDF = 4096;
constexpr bool is_vort_resid(int MASK) { return MASK == ORDN || MASK == ORDF; }
// THE NETWORK INPUTS (mask == ORDI or ORDJ, alone; D == 2; forward only): the four arrays that the reference's
// Model.forward hands to its dynamics network (model_pn.py:645-664), each through its own output slot,
//   o0[m][ch]          = u                                   sample_u    [M][c]
//   o1[m][i][ch]       = d_i u_ch                            sample_ux   [M][2c], the memory of order 1
//   o2[m][0][ch], [1]  = u_xx, u_yy                          sample_uxx  [M][2c], planar (the cat of :664)
//   o3[m][..]          = pde_rhs (:612-631) by NetIn::kind   sample_pde  [M][p]
// Of the Hessian only the diagonal is wanted and of the third derivative only lap w, so ORDI accumulates u, +sum p w
// and the two diagonal second derivatives (5 c sums, no t_xy) and ORDJ (C == 2) those ten and w_x, w_y, lap w formed
// per pair as ORDV forms them: 13 sums against the 30 of orders 0..3.  pde_rhs holds products of two such sums (u u_x,
// u . grad w), so it is composed once per point in fwd_store.  The kind is a run-time field: the store runs once per point.
constexpr int ORDI = 1024;      // kinds zero, diffusion, burgers, wave
constexpr int ORDJ = 2048;      // kind navier_stokes
constexpr bool is_net_inputs(int MASK) { return MASK == ORDI || MASK == ORDJ; }
constexpr int NET_ZERO = 0, NET_DIFFUSION = 1, NET_BURGERS = 2, NET_WAVE = 3, NET_NAVIER_STOKES = 4;      // PIGS_NET_* of the C ABI
constexpr int NNETJ = 13;
template <typename T> struct NetIn {
    int kind;
    T nu, wave[2];
};
// host side: the block from the C ABI's PigsNetworkInputs (include/pigs_amd.h) in the launch's type
template <typename T, typename ABI>
inline NetIn<T> make_net_in(const ABI& t) {
    return NetIn<T>{t.kind, (T)t.nu, {(T)t.wave[0], (T)t.wave[1]}};
}
constexpr int bwd_mask_of(int MASK) {
    return (MASK == ORDR || MASK == ORDG) ? ORDR_AS : (MASK == ORDV || is_vort_resid(MASK)) ? ORDV_AS : MASK == ORDC ? ORDC_AS : MASK;
}

template <typename T> struct Terms {
    T a0, a1[2], aL, adv;                           // used where the field pointer is null
    T B[2][4];                                      // advect_by[i][c']
    const T *a0_pt, *a1_pt, *aL_pt, *adv_pt;        // per-point fields [M], [M][d], [M], [M] or null
    const T* target;                                // [M][c] or null
    T* aux;                                         // [M][1+d][c]: written by the forward, read by the backward; or null
};
// host side: the block from the C ABI's PigsResidualTerms (include/pigs_amd.h) in the launch's type
template <typename T, typename ABI>
inline Terms<T> make_terms(const ABI& t, const void* target, const void* aux) {
    Terms<T> z{};
    z.a0 = (T)t.a0; z.a1[0] = (T)t.a1[0]; z.a1[1] = (T)t.a1[1]; z.aL = (T)t.aL; z.adv = (T)t.adv;
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 4; ++k) z.B[i][k] = (T)t.advect_by[i][k];
    z.a0_pt = (const T*)t.a0_pt; z.a1_pt = (const T*)t.a1_pt; z.aL_pt = (const T*)t.aL_pt; z.adv_pt = (const T*)t.adv_pt;
    z.target = (const T*)target;
    z.aux = (T*)const_cast<void*>(aux);
    return z;
}
template <typename T> struct Coupled {
    T a0, aL, cw;                                   // used where the field pointer is null
    T Q0[4][4], QL[4][4];                           // couple0[ch][c'], couple_lap[ch][c']
    const T *a0_pt, *aL_pt, *cw_pt;                 // per-point fields [M] or null
    const T* target;                                // [M][c] or null
};
// host side: the block from the C ABI's PigsResidualCoupling (include/pigs_amd.h) in the launch's type
template <typename T, typename ABI>
inline Coupled<T> make_coupled(const ABI& t, const void* target) {
    Coupled<T> z{};
    z.a0 = (T)t.a0; z.aL = (T)t.aL; z.cw = (T)t.cw;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) { z.Q0[i][k] = (T)t.couple0[i][k]; z.QL[i][k] = (T)t.couple_lap[i][k]; }
    z.a0_pt = (const T*)t.a0_pt; z.aL_pt = (const T*)t.aL_pt; z.cw_pt = (const T*)t.cw_pt;
    z.target = (const T*)target;
    return z;
}
template <typename T> struct VortResid {
    T nu, dt, time_term, tau;                       // tau: used where tau_pt is null
    const T* tau_pt;                                // [M] or null
    const T* prev;                                  // [M][7], the previous time level's vorticity terms; or null (zeros)
    T* aux;                                         // [M][4]: written by the forward, read by the backward; or null
};
// host side: the block from the C ABI's PigsVorticityResidual (include/pigs_amd.h) in the launch's type
template <typename T, typename ABI>
inline VortResid<T> make_vort_resid(const ABI& t, const void* prev, const void* aux) {
    VortResid<T> z{};
    z.nu = (T)t.nu; z.dt = (T)t.dt; z.time_term = (T)t.time_term; z.tau = (T)t.tau;
    z.tau_pt = (const T*)t.tau_pt;
    z.prev = (const T*)prev;
    z.aux = (T*)const_cast<void*>(aux);
    return z;
}
// the vorticity fit: the vorticity residual's block, the data and its weight
template <typename T> struct VortFit : VortResid<T> {
    const T* data;                                  // [M]; read by the forward alone
    T data_weight;
};
// host side: the block from the C ABI's PigsVorticityFit (include/pigs_amd.h) in the launch's type
template <typename T, typename ABI>
inline VortFit<T> make_vort_fit(const ABI& t, const void* prev, const void* aux, bool backward) {
    VortFit<T> z{};
    static_cast<VortResid<T>&>(z) = make_vort_resid<T>(t, prev, aux);
    z.data = backward ? nullptr : (const T*)t.data;
    z.data_weight = (T)t.data_weight;
    return z;
}
// the coefficient block a kernel compiled for MASK receives
template <typename T, int MASK>
using RzOf = std::conditional_t<MASK == ORDG, Terms<T>, std::conditional_t<MASK == ORDC, Coupled<T>,
             std::conditional_t<MASK == ORDN, VortResid<T>, std::conditional_t<MASK == ORDF, VortFit<T>,
             std::conditional_t<is_net_inputs(MASK), NetIn<T>, Resid<T>>>>>>;
// host side: that block from a launcher's arguments (launch.h's SampleArgs; aux: the forward's output, the backward's
// input; the target / previous level is read by the forward alone)
template <typename T, int MASK, typename ARGS>
inline RzOf<T, MASK> rz_of(const ARGS& a, bool backward) {
    if constexpr (MASK == ORDG) {
        return make_terms<T>(*a.terms, backward ? nullptr : a.target, a.aux);
    } else if constexpr (MASK == ORDC) {
        return make_coupled<T>(*a.coupling, backward ? nullptr : a.target);
    } else if constexpr (MASK == ORDN) {
        return make_vort_resid<T>(*a.vort, backward ? nullptr : a.target, a.aux);
    } else if constexpr (MASK == ORDF) {
        return make_vort_fit<T>(*a.fit, backward ? nullptr : a.target, a.aux, backward);
    } else if constexpr (is_net_inputs(MASK)) {
        return make_net_in<T>(*a.net);
    } else {
        return Resid<T>{(T)a.resid[0], {(T)a.resid[1], (T)a.resid[2]}, (T)a.resid[3], backward ? nullptr : (const T*)a.target};
    }
}

// the coefficients of the general residual at one point
template <typename T, int D> struct TermsAt {
    T a0, a1[D], aL, adv;
    __device__ __forceinline__ void load(const Terms<T>& tz, int64_t m) {
        a0 = tz.a0_pt ? tz.a0_pt[m] : tz.a0;
#pragma unroll
        for (int i = 0; i < D; ++i) a1[i] = tz.a1_pt ? tz.a1_pt[m * D + i] : tz.a1[i];
        aL = tz.aL_pt ? tz.aL_pt[m] : tz.aL;
        adv = tz.adv_pt ? tz.adv_pt[m] : tz.adv;
    }
};

template <int D> struct Sym {
    static constexpr int NF = D * (D + 1) / 2;            // distinct 2nd-order components
    static constexpr int N3 = D * (D + 1) * (D + 2) / 6;  // distinct 3rd-order components
};

template <typename T> __device__ __forceinline__ T exp_neg_half(T q);
template <> __device__ __forceinline__ float exp_neg_half<float>(float q) {
    // v_exp_f32 on a pre-scaled argument: exp(-q/2) = 2^(-q * log2(e)/2)
#ifdef PIGS_EXP_SCALE_VGPR
    float k;          // the factor from a register instead of a 32-bit literal (no "volatile": hoisted out of loops)
    asm("v_mov_b32 %0, 0xbf38aa3b" : "=v"(k));
    return __builtin_amdgcn_exp2f(q * k);
#else
    return __builtin_amdgcn_exp2f(q * -0.72134752044448170368f);
#endif
}
template <> __device__ __forceinline__ double exp_neg_half<double>(double q) { return exp(-0.5 * q); }

template <typename T> __device__ __forceinline__ T fma_(T a, T b, T c) { return __builtin_fma(a, b, c); }
template <> __device__ __forceinline__ float fma_<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// Layout of the flat forward accumulator array for a compile-time order mask.
template <int D, int C, int MASK_> struct FwdLayout {
    // the general residual accumulates u, grad u, trace; the coupled one u and the trace
    static constexpr int MASK = MASK_ == ORDG ? ORDR_AS : MASK_ == ORDC ? ORDC_AS : MASK_;
    static constexpr int O0 = 0;
    static constexpr int O1 = O0 + ((MASK & ORD0) ? C : 0);
    static constexpr int O2 = O1 + ((MASK & ORD1) ? D * C : 0);
    static constexpr int O3 = O2 + ((MASK & ORD2) ? Sym<D>::NF * C : (MASK & ORD2T) ? C : 0);
    static constexpr int N = O3 + ((MASK & ORD3) ? Sym<D>::N3 * C : 0) + ((MASK & ORDR) ? C : 0) + ((MASK == ORDV || is_vort_resid(MASK)) ? NVORT : 0) +
                             (MASK == ORDI ? 5 * C : MASK == ORDJ ? NNETJ : 0);
    // the network inputs (D = 2): u, +sum p_i w, t_xx w, t_yy w per channel; ORDJ: w_x, w_y, lap w behind them
    static constexpr int IU = 0, IP = C, IXX = 3 * C, IYY = 4 * C, IW = 5 * C;
};

// Pair geometry: x, p, g (and nothing else) for one (point, Gaussian).
template <typename T, int D> struct Pair {
    T x[D], p[D], g;
    __device__ __forceinline__ void eval(const T* s, const T* mu, const T* con) {
        if constexpr (D == 1) {
            x[0] = s[0] - mu[0];
            p[0] = con[0] * x[0];
            g = exp_neg_half<T>(x[0] * p[0]);
        } else {
            x[0] = s[0] - mu[0];
            x[1] = s[1] - mu[1];
            p[0] = fma_<T>(con[1], x[1], con[0] * x[0]);
            p[1] = fma_<T>(con[2], x[1], con[1] * x[0]);
            g = exp_neg_half<T>(fma_<T>(x[1], p[1], x[0] * p[0]));
        }
    }
};

// acc += contributions of one Gaussian to the outputs selected by MASK at one sample point.
// The order-1 accumulator holds +sum(p w); the sign is applied on store.
template <typename T, int D, int C, int MASK>
__device__ __forceinline__ void fwd_accumulate(T* acc, const T* s, const T* mu, const T* con, const T* v,
                                               const RzOf<T, MASK>* rz = nullptr) {
    if constexpr (MASK == ORDG) {
        fwd_accumulate<T, D, C, ORDR_AS>(acc, s, mu, con, v);
        return;
    }
    if constexpr (MASK == ORDC) {
        fwd_accumulate<T, D, C, ORDC_AS>(acc, s, mu, con, v);
        return;
    }
    if constexpr (is_vort_resid(MASK)) {      // the seven sums of the vorticity terms, their `live` guard included
        fwd_accumulate<T, D, C, ORDV>(acc, s, mu, con, v);
        return;
    }
    using L = FwdLayout<D, C, MASK>;
    Pair<T, D> pr;
    pr.eval(s, mu, con);
    if constexpr (MASK == ORDR) {
        // one polynomial factor per pair, one accumulator per channel: a0 - a1 . p + aL (|p|^2 - tr C)
        T F;
        if constexpr (D == 1) {
            F = fma_<T>(rz->aL, fma_<T>(pr.p[0], pr.p[0], -con[0]), fma_<T>(-rz->a1[0], pr.p[0], rz->a0));
        } else {
            const T ttr = fma_<T>(pr.p[0], pr.p[0], fma_<T>(pr.p[1], pr.p[1], -(con[0] + con[2])));
            F = fma_<T>(rz->aL, ttr, fma_<T>(-rz->a1[0], pr.p[0], fma_<T>(-rz->a1[1], pr.p[1], rz->a0)));
        }
        const T Fg = F * pr.g;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) acc[ch] = fma_<T>(v[ch], Fg, acc[ch]);
        return;
    }
    if constexpr (MASK == ORDV) {
        static_assert(D == 2 && C == 2, "the vorticity terms are those of a two-channel field in two dimensions");
        // the guard of ORD3 below: an underflowed g must not meet an overflowing cubic (L_k)
        const bool live = pr.g > T(0);
        const T px = live ? pr.p[0] : T(0), py = live ? pr.p[1] : T(0);
        const T txx = fma_<T>(px, px, -con[0]), txy = fma_<T>(px, py, -con[1]), tyy = fma_<T>(py, py, -con[2]);
        // L_k = sum_i t3_iik = 2 (C p)_k - (|p|^2 - tr C) p_k     (t3_ijk = C_ij p_k + C_ik p_j + C_jk p_i - p_i p_j p_k)
        const T ttr = txx + tyy;
        const T Lx = fma_<T>(T(2), fma_<T>(con[0], px, con[1] * py), -ttr * px);
        const T Ly = fma_<T>(T(2), fma_<T>(con[1], px, con[2] * py), -ttr * py);
        const T wx = v[0] * pr.g, wy = v[1] * pr.g;      // d_i u_ch = -p_i w_ch, d_i d_j u_ch = t_ij w_ch
        acc[0] += wx;
        acc[1] += wy;
        acc[2] = fma_<T>(-px, wx, fma_<T>(-py, wy, acc[2]));      // d_x u_x + d_y u_y
        acc[3] = fma_<T>(py, wx, fma_<T>(-px, wy, acc[3]));       // d_x u_y - d_y u_x
        acc[4] = fma_<T>(txx, wy, fma_<T>(-txy, wx, acc[4]));     // d_x w
        acc[5] = fma_<T>(txy, wy, fma_<T>(-tyy, wx, acc[5]));     // d_y w
        acc[6] = fma_<T>(Lx, wy, fma_<T>(-Ly, wx, acc[6]));       // lap w
        return;
    }
    if constexpr (is_net_inputs(MASK)) {
        static_assert(D == 2, "the network inputs are those of the reference's two-dimensional model");
        static_assert(MASK == ORDI || C == 2, "the Navier-Stokes right-hand side is that of a two-channel field");
        T px = pr.p[0], py = pr.p[1];
        if constexpr (MASK == ORDJ) {      // the guard of ORDV above: an underflowed g must not meet an overflowing cubic
            const bool live = pr.g > T(0);
            px = live ? px : T(0);
            py = live ? py : T(0);
        }
        const T txx = fma_<T>(px, px, -con[0]), tyy = fma_<T>(py, py, -con[2]);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const T w = v[ch] * pr.g;
            acc[L::IU + ch] += w;
            acc[L::IP + ch] = fma_<T>(px, w, acc[L::IP + ch]);
            acc[L::IP + C + ch] = fma_<T>(py, w, acc[L::IP + C + ch]);
            acc[L::IXX + ch] = fma_<T>(txx, w, acc[L::IXX + ch]);
            acc[L::IYY + ch] = fma_<T>(tyy, w, acc[L::IYY + ch]);
        }
        if constexpr (MASK == ORDJ) {      // grad w and lap w, as ORDV forms them
            const T txy = fma_<T>(px, py, -con[1]);
            const T ttr = txx + tyy;
            const T Lx = fma_<T>(T(2), fma_<T>(con[0], px, con[1] * py), -ttr * px);
            const T Ly = fma_<T>(T(2), fma_<T>(con[1], px, con[2] * py), -ttr * py);
            const T wx = v[0] * pr.g, wy = v[1] * pr.g;
            acc[L::IW + 0] = fma_<T>(txx, wy, fma_<T>(-txy, wx, acc[L::IW + 0]));     // d_x w
            acc[L::IW + 1] = fma_<T>(txy, wy, fma_<T>(-tyy, wx, acc[L::IW + 1]));     // d_y w
            acc[L::IW + 2] = fma_<T>(Lx, wy, fma_<T>(-Ly, wx, acc[L::IW + 2]));       // lap w
        }
        return;
    }
    if constexpr ((MASK & ORD3) != 0) {
        // a pair whose g has underflowed to zero contributes nothing, but its cubic factor can
        // overflow (|p| > 7e12: conics of 1e12 from |rho| -> 1) and 0 * inf would poison the sum
        const bool live = pr.g > T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) pr.p[i] = live ? pr.p[i] : T(0);
    }
    if constexpr (D == 1) {
        const T p = pr.p[0];
        T t2 = 0, t3 = 0;
        if constexpr ((MASK & (ORD2 | ORD2T | ORD3)) != 0) t2 = fma_<T>(p, p, -con[0]);
        if constexpr ((MASK & ORD3) != 0) t3 = p * (T(2) * con[0] - t2);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const T w = v[ch] * pr.g;
            if constexpr ((MASK & ORD0) != 0) acc[L::O0 + ch] += w;
            if constexpr ((MASK & ORD1) != 0) acc[L::O1 + ch] = fma_<T>(p, w, acc[L::O1 + ch]);
            if constexpr ((MASK & (ORD2 | ORD2T)) != 0) acc[L::O2 + ch] = fma_<T>(t2, w, acc[L::O2 + ch]);   // d = 1: trace = u_xx
            if constexpr ((MASK & ORD3) != 0) acc[L::O3 + ch] = fma_<T>(t3, w, acc[L::O3 + ch]);
        }
    } else {
        const T px = pr.p[0], py = pr.p[1];
        T txx = 0, txy = 0, tyy = 0, t3[4] = {0, 0, 0, 0};
        if constexpr ((MASK & (ORD2 | ORD3)) != 0) {
            txx = fma_<T>(px, px, -con[0]);
            tyy = fma_<T>(py, py, -con[2]);
        }
        if constexpr ((MASK & ORD2) != 0) txy = fma_<T>(px, py, -con[1]);
        T ttr = 0;      // |p|^2 - tr C
        if constexpr ((MASK & ORD2T) != 0) {
            if constexpr ((MASK & ORD3) != 0) ttr = txx + tyy;
            else ttr = fma_<T>(px, px, fma_<T>(py, py, -(con[0] + con[2])));
        }
        if constexpr ((MASK & ORD3) != 0) {
            // C_ij p_k + C_ik p_j + C_jk p_i - p_i p_j p_k, written through t_ij = p_i p_j - C_ij
            const T b2 = T(2) * con[1];
            t3[0] = px * (T(2) * con[0] - txx);   // xxx = 3a px - px^3
            t3[1] = fma_<T>(b2, px, -txx * py);   // xxy = 2b px + a py - px^2 py
            t3[2] = fma_<T>(b2, py, -tyy * px);   // xyy = c px + 2b py - px py^2
            t3[3] = py * (T(2) * con[2] - tyy);   // yyy = 3c py - py^3
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const T w = v[ch] * pr.g;
            if constexpr ((MASK & ORD0) != 0) acc[L::O0 + ch] += w;
            if constexpr ((MASK & ORD1) != 0) {
                acc[L::O1 + 0 * C + ch] = fma_<T>(px, w, acc[L::O1 + 0 * C + ch]);
                acc[L::O1 + 1 * C + ch] = fma_<T>(py, w, acc[L::O1 + 1 * C + ch]);
            }
            if constexpr ((MASK & ORD2) != 0) {
                acc[L::O2 + 0 * C + ch] = fma_<T>(txx, w, acc[L::O2 + 0 * C + ch]);
                acc[L::O2 + 1 * C + ch] = fma_<T>(txy, w, acc[L::O2 + 1 * C + ch]);
                acc[L::O2 + 2 * C + ch] = fma_<T>(tyy, w, acc[L::O2 + 2 * C + ch]);
            }
            if constexpr ((MASK & ORD2T) != 0) acc[L::O2 + ch] = fma_<T>(ttr, w, acc[L::O2 + ch]);
            if constexpr ((MASK & ORD3) != 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[L::O3 + k * C + ch] = fma_<T>(t3[k], w, acc[L::O3 + k * C + ch]);
            }
        }
    }
}

// Expand the symmetric accumulators into the reference layouts
//   out0[M][c], out1[M][d][c], out2[M][d][d][c], out3[M][d][d][d][c]
// for point m.  Null output pointers are skipped (the order was computed but not requested).
// STREAM: non-temporal stores (`nt`): outputs that nothing in the launch reads again leave the L2 as
// they are written instead of staying dirty until the end-of-kernel write-back (the binned forward at
// C3 writes 24 MB: 28.0 -> 26.6 us); the dense kernels' small outputs stay cacheable for the consumer.
template <bool STREAM, typename T>
__device__ __forceinline__ void store_out(T* p, T v) {
    if constexpr (STREAM) __builtin_nontemporal_store(v, p);
    else *p = v;
}
template <typename T, int D, int C, int MASK, bool STREAM = false>
__device__ __forceinline__ void fwd_store(const T* acc, int64_t m, T* __restrict__ o0, T* __restrict__ o1,
                                          T* __restrict__ o2, T* __restrict__ o3, const RzOf<T, MASK>* rz = nullptr) {
    using L = FwdLayout<D, C, MASK>;
    if constexpr (MASK == ORDG) {
        // the composing store: the point's coefficients and target meet its finished sums
        TermsAt<T, D> k;
        k.load(*rz, m);
        T coef[D];      // a1_i + adv w_i
#pragma unroll
        for (int i = 0; i < D; ++i) {
            T w = T(0);
#pragma unroll
            for (int cc = 0; cc < C; ++cc) w = fma_<T>(rz->B[i][cc], acc[L::O0 + cc], w);
            coef[i] = fma_<T>(k.adv, w, k.a1[i]);
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            T r = fma_<T>(k.aL, acc[L::O2 + ch], k.a0 * acc[L::O0 + ch]);
#pragma unroll
            for (int i = 0; i < D; ++i) r = fma_<T>(-coef[i], acc[L::O1 + i * C + ch], r);      // the accumulator holds -d_i u
            store_out<STREAM>(&o0[m * C + ch], rz->target ? r - rz->target[m * C + ch] : r);
        }
        if (rz->aux) {
            T* ax = rz->aux + m * (1 + D) * C;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) store_out<STREAM>(&ax[ch], acc[L::O0 + ch]);
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) store_out<STREAM>(&ax[(1 + i) * C + ch], -acc[L::O1 + i * C + ch]);
        }
        return;
    }
    if constexpr (MASK == ORDC) {
        // the composing store: the point's three coefficients, the two matrices (kernel arguments) and the target
        const T a0 = rz->a0_pt ? rz->a0_pt[m] : rz->a0, aL = rz->aL_pt ? rz->aL_pt[m] : rz->aL;
        const T cw = rz->cw_pt ? rz->cw_pt[m] : rz->cw;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            T mix = T(0);
#pragma unroll
            for (int cc = 0; cc < C; ++cc)
                mix = fma_<T>(rz->Q0[ch][cc], acc[L::O0 + cc], fma_<T>(rz->QL[ch][cc], acc[L::O2 + cc], mix));
            const T r = fma_<T>(cw, mix, fma_<T>(aL, acc[L::O2 + ch], a0 * acc[L::O0 + ch]));
            store_out<STREAM>(&o0[m * C + ch], rz->target ? r - rz->target[m * C + ch] : r);
        }
        return;
    }
    if constexpr (is_vort_resid(MASK)) {
        // the composing store: the point's tau and its row of the previous level meet the seven finished sums
        static_assert(D == 2 && C == 2, "the vorticity residual is that of a two-channel field in two dimensions");
        const T tau = rz->tau_pt ? rz->tau_pt[m] : rz->tau;
        T pv[NVORT];
#pragma unroll
        for (int k = 0; k < NVORT; ++k) pv[k] = rz->prev ? rz->prev[m * NVORT + k] : T(0);
        const T om = T(1) - tau;
        T b[NVORT];      // the blend; b[3] (w) is not one: the time term takes the difference of the levels
#pragma unroll
        for (int k = 0; k < NVORT; ++k) b[k] = fma_<T>(tau, acc[k], om * pv[k]);
        const T adv = fma_<T>(b[0], b[4], b[1] * b[5]);      // u_b . grad w_b
        const T r = fma_<T>(rz->time_term, acc[3] - pv[3], -rz->dt * fma_<T>(rz->nu, b[6], -adv));
        if constexpr (STREAM) asm volatile("" ::: "memory");      // as for ORDV below: keeps the hint
        if constexpr (MASK == ORDF) {
            // three adjacent words; the point's data word is fetched here, after r, when prev's row is dead
            const T fit = rz->data_weight * (acc[3] - rz->data[m]);
            store_out<STREAM>(&o0[m * 3], b[2]);
            store_out<STREAM>(&o0[m * 3 + 1], r);
            store_out<STREAM>(&o0[m * 3 + 2], fit);
        } else {
            store_out<STREAM>(&o0[m * 2], b[2]);
            store_out<STREAM>(&o0[m * 2 + 1], r);
        }
        if (rz->aux) {
            T* ax = rz->aux + m * 4;
            store_out<STREAM>(&ax[0], b[0]);
            store_out<STREAM>(&ax[1], b[1]);
            store_out<STREAM>(&ax[2], b[4]);
            store_out<STREAM>(&ax[3], b[5]);
        }
        return;
    }
    if constexpr (MASK == ORDR) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
            store_out<STREAM>(&o0[m * C + ch], rz->target ? acc[ch] - rz->target[m * C + ch] : acc[ch]);
        return;
    }
    if constexpr (is_net_inputs(MASK)) {
        // the composing store: the four arrays of Model.forward in their layouts (:650-664), pde_rhs by kind (:612-631)
        if constexpr (STREAM) asm volatile("" ::: "memory");      // as for ORDV below: keeps the hint
#pragma unroll
        for (int ch = 0; ch < C; ++ch) store_out<STREAM>(&o0[m * C + ch], acc[L::IU + ch]);
#pragma unroll
        for (int k = 0; k < 2 * C; ++k) store_out<STREAM>(&o1[m * 2 * C + k], -acc[L::IP + k]);      // the sign of order 1
#pragma unroll
        for (int k = 0; k < 2 * C; ++k) store_out<STREAM>(&o2[m * 2 * C + k], acc[L::IXX + k]);       // u_xx of every channel, then u_yy
        if constexpr (MASK == ORDJ) {
            // nu lap w - (u_0 w_x + u_1 w_y)
            const T adv = fma_<T>(acc[L::IU + 0], acc[L::IW + 0], acc[L::IU + 1] * acc[L::IW + 1]);
            store_out<STREAM>(&o3[m], fma_<T>(rz->nu, acc[L::IW + 2], -adv));
        } else if (rz->kind == NET_WAVE) {
            // (u_1, wave_0 lap u_0 - wave_1 u_1): two channels, which the entry point has checked
            if constexpr (C == 2) {
                const T lap0 = acc[L::IXX + 0] + acc[L::IYY + 0];
                store_out<STREAM>(&o3[m * 2 + 0], acc[L::IU + 1]);
                store_out<STREAM>(&o3[m * 2 + 1], fma_<T>(rz->wave[0], lap0, -rz->wave[1] * acc[L::IU + 1]));
            }
        } else {
            // zero; lap u; nu lap u - u_ch d_x u_ch (the accumulator holds -d_x u)
            const int kind = rz->kind;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const T lap = acc[L::IXX + ch] + acc[L::IYY + ch];
                const T burgers = fma_<T>(rz->nu, lap, acc[L::IU + ch] * acc[L::IP + ch]);
                store_out<STREAM>(&o3[m * C + ch], kind == NET_DIFFUSION ? lap : kind == NET_BURGERS ? burgers : T(0));
            }
        }
        return;
    }
    if constexpr (MASK == ORDV) {
        // one packed row of seven adjacent words (word-aligned only): the compiler joins them into a four-word and a
        // three-word store (checked in the ISA: global_store_dwordx4 + global_store_dwordx3, `nt` under STREAM)
        // (the empty asm: a caller with a streamed and a plain branch would otherwise see the two branches' identical
        // unconditional stores hoisted into one, which loses the hint)
        T* row = o0 + m * NVORT;
        if constexpr (STREAM) asm volatile("" ::: "memory");
#pragma unroll
        for (int k = 0; k < NVORT; ++k) store_out<STREAM>(&row[k], acc[k]);
        return;
    }
    if constexpr ((MASK & ORD0) != 0) {
        if (o0) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) store_out<STREAM>(&o0[m * C + ch], acc[L::O0 + ch]);
        }
    }
    if constexpr ((MASK & ORD1) != 0) {
        if (o1) {
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) store_out<STREAM>(&o1[(m * D + i) * C + ch], -acc[L::O1 + i * C + ch]);
        }
    }
    if constexpr ((MASK & ORD2) != 0) {
        if (o2) {
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j)
#pragma unroll
                    for (int ch = 0; ch < C; ++ch)
                        store_out<STREAM>(&o2[((m * D + i) * D + j) * C + ch], acc[L::O2 + (i + j) * C + ch]);  // D<=2: sym index = i+j
        }
    }
    if constexpr ((MASK & ORD2T) != 0) {      // trace: out2 is [M][c]
        if (o2) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) store_out<STREAM>(&o2[m * C + ch], acc[L::O2 + ch]);
        }
    }
    if constexpr ((MASK & ORD3) != 0) {
        if (o3) {
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j)
#pragma unroll
                    for (int k = 0; k < D; ++k)
#pragma unroll
                        for (int ch = 0; ch < C; ++ch)
                            store_out<STREAM>(&o3[(((m * D + i) * D + j) * D + k) * C + ch], acc[L::O3 + (i + j + k) * C + ch]);
        }
    }
}

// Inverse of fwd_store: read the partial sums of point m back into the accumulators (a cell with
// more than 64 points evaluates each queue flush for every 64-point chunk and parks the partial
// sums in the output rows in between).  Null outputs were never stored and are not wanted: zero.
template <typename T, int D, int C, int MASK>
__device__ __forceinline__ void fwd_load(T* acc, int64_t m, const T* __restrict__ o0, const T* __restrict__ o1,
                                         const T* __restrict__ o2, const T* __restrict__ o3) {
    using L = FwdLayout<D, C, MASK>;
#pragma unroll
    for (int k = 0; k < L::N; ++k) acc[k] = T(0);
    if constexpr (MASK == ORDV) {      // the accumulators are the outputs
#pragma unroll
        for (int k = 0; k < NVORT; ++k) acc[k] = o0[m * NVORT + k];
        return;
    }
    if constexpr ((MASK & ORD0) != 0) {
        if (o0) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[L::O0 + ch] = o0[m * C + ch];
        }
    }
    if constexpr ((MASK & ORD1) != 0) {
        if (o1) {
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) acc[L::O1 + i * C + ch] = -o1[(m * D + i) * C + ch];
        }
    }
    if constexpr ((MASK & ORD2) != 0) {
        if (o2) {
#pragma unroll
            for (int k = 0; k < Sym<D>::NF; ++k)        // (0,0), (0,1), (1,1): first index 0 until the last
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const int i = k == Sym<D>::NF - 1 ? D - 1 : 0, j = k - i;
                    acc[L::O2 + k * C + ch] = o2[((m * D + i) * D + j) * C + ch];
                }
        }
    }
    if constexpr ((MASK & ORD2T) != 0) {
        if (o2) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[L::O2 + ch] = o2[m * C + ch];
        }
    }
    if constexpr ((MASK & ORD3) != 0) {
        if (o3) {
#pragma unroll
            for (int k = 0; k < Sym<D>::N3; ++k)        // (0,0,0), (0,0,1), (0,1,1), (1,1,1)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const int a = k >= 3 ? 1 : 0, b = k >= 2 ? 1 : 0, c3 = k >= 1 ? 1 : 0;     // D = 2
                    const int i = D == 1 ? 0 : a, j = D == 1 ? 0 : b, l = D == 1 ? 0 : c3;
                    acc[L::O3 + k * C + ch] = o3[(((m * D + i) * D + j) * D + l) * C + ch];
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Backward (VJP) of the selected outputs wrt (means, flat conics, values) for one pair.
//
//   L = sum_m sum_n g sum_c v_c F_c ,  F_c = G0_c - G1_ic p_i + H_ij,c t_ij + K_ijk,c poly3_ijk
// with the incoming gradients symmetrised once per point (Gsym below).  With A = sum_c v_c F_c,
// dA = grad_p A and E = explicit dA/dC:
//   dL/dv_c   += g F_c
//   dL/dmu_l  += g (A p_l - sum_i dA_i C_il)
//   dL/dC_kl  += g (-A x_k x_l / 2 + dA_k x_l + E_kl)      (full matrix; flat = [00, 01+10, 11])
// This is what torch.autograd gives through the reference functions
// (test_derivatives.py:122-124, 208-220, 340-356).
// ---------------------------------------------------------------------------------------------

// Incoming gradients at one sample point, symmetrised over derivative indices.
template <typename T, int D, int C, int MASK> struct Gsym {
    T g0[C], g1[D][C], g2[Sym<D>::NF][C], g3[Sym<D>::N3][C];
    // Null gradient pointers (an order inside the compiled mask whose output received no
    // gradient) read as zero.
    __device__ __forceinline__ void load(int64_t m, const T* __restrict__ G0, const T* __restrict__ G1,
                                         const T* __restrict__ G2, const T* __restrict__ G3) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            if constexpr ((MASK & ORD0) != 0) g0[ch] = G0 ? G0[m * C + ch] : T(0);
            if constexpr ((MASK & ORD1) != 0) {
#pragma unroll
                for (int i = 0; i < D; ++i) g1[i][ch] = G1 ? G1[(m * D + i) * C + ch] : T(0);
            }
            if constexpr ((MASK & ORD2) != 0) {
#pragma unroll
                for (int k = 0; k < Sym<D>::NF; ++k) g2[k][ch] = 0;
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) g2[i + j][ch] += G2 ? G2[((m * D + i) * D + j) * C + ch] : T(0);
            }
            if constexpr ((MASK & ORD2T) != 0) {   // gradient of the trace = gl * identity
                const T gl = G2 ? G2[m * C + ch] : T(0);
#pragma unroll
                for (int k = 0; k < Sym<D>::NF; ++k) g2[k][ch] = (k == 0 || k == Sym<D>::NF - 1) ? gl : T(0);
            }
            if constexpr ((MASK & ORD3) != 0) {
#pragma unroll
                for (int k = 0; k < Sym<D>::N3; ++k) g3[k][ch] = 0;
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j)
#pragma unroll
                        for (int k = 0; k < D; ++k)
                            g3[i + j + k][ch] += G3 ? G3[(((m * D + i) * D + j) * D + k) * C + ch] : T(0);
            }
        }
    }
    // the incoming gradient gr [M][c] of a residual output (MASK = ORDR_AS): g0 = a0 gr, g1 = a1 gr, trace = aL gr
    __device__ __forceinline__ void load_residual(int64_t m, const T* __restrict__ GR, const Resid<T>& rz) {
        static_assert(MASK == ORDR_AS, "a residual's backward runs on orders 0, 1 and the trace");
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const T gr = GR[m * C + ch];
            g0[ch] = rz.a0 * gr;
#pragma unroll
            for (int i = 0; i < D; ++i) g1[i][ch] = rz.a1[i] * gr;
#pragma unroll
            for (int k = 0; k < Sym<D>::NF; ++k) g2[k][ch] = (k == 0 || k == Sym<D>::NF - 1) ? rz.aL * gr : T(0);
        }
    }
    // the incoming gradient gr [M][c] of a coupled residual (MASK = ORDC_AS) with the point's coefficients a0, aL, cw:
    //   g0[c'] = a0 gr_c' + cw sum_ch Q0[ch][c'] gr_ch,  trace[c'] = aL gr_c' + cw sum_ch QL[ch][c'] gr_ch
    __device__ __forceinline__ void form_coupled(const T* gr, T a0, T aL, T cw, const Coupled<T>& cz) {
        static_assert(MASK == ORDC_AS, "a coupled residual's backward runs on order 0 and the trace");
#pragma unroll
        for (int cc = 0; cc < C; ++cc) {
            T m0 = T(0), mL = T(0);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                m0 = fma_<T>(cz.Q0[ch][cc], gr[ch], m0);
                mL = fma_<T>(cz.QL[ch][cc], gr[ch], mL);
            }
            g0[cc] = fma_<T>(cw, m0, a0 * gr[cc]);
            const T tr = fma_<T>(cw, mL, aL * gr[cc]);
#pragma unroll
            for (int k = 0; k < Sym<D>::NF; ++k) g2[k][cc] = (k == 0 || k == Sym<D>::NF - 1) ? tr : T(0);
        }
    }
    // the same with everything read at point m
    __device__ __forceinline__ void load_coupled(int64_t m, const T* __restrict__ GR, const Coupled<T>& cz) {
        T gr[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) gr[ch] = GR[m * C + ch];
        form_coupled(gr, cz.a0_pt ? cz.a0_pt[m] : cz.a0, cz.aL_pt ? cz.aL_pt[m] : cz.aL, cz.cw_pt ? cz.cw_pt[m] : cz.cw, cz);
    }
    // the incoming gradient gv [M][7] of the vorticity terms (MASK = ORDV_AS, D = 2, C = 2) as the gradients that arrive
    // at orders 0..3, in this struct's symmetric components (g2[i + j], g3[i + j + k]: each the SUM over the index
    // orders that share it):
    //   div = o1[0][0] + o1[1][1],  w = o1[0][1] - o1[1][0],  w_i = o2[i][0][1] - o2[i][1][0],
    //   lap w = sum_i o3[i][i][0][1] - o3[i][i][1][0]                                (last index: the channel)
    __device__ __forceinline__ void load_vorticity(int64_t m, const T* __restrict__ GV) {
        static_assert(MASK == ORDV_AS && D == 2 && C == 2, "the vorticity terms' backward runs on orders 0..3 of d = 2, c = 2");
        T gv[NVORT];
#pragma unroll
        for (int k = 0; k < NVORT; ++k) gv[k] = GV[m * NVORT + k];
        form_vorticity(gv);
    }
    // the same from the seven numbers in registers
    __device__ __forceinline__ void form_vorticity(const T* gv) {
        static_assert(MASK == ORDV_AS && D == 2 && C == 2, "the vorticity terms' backward runs on orders 0..3 of d = 2, c = 2");
        g0[0] = gv[0];          g0[1] = gv[1];
        g1[0][0] = gv[2];       g1[0][1] = gv[3];
        g1[1][0] = -gv[3];      g1[1][1] = gv[2];
        g2[0][0] = T(0);        g2[0][1] = gv[4];      // xx
        g2[1][0] = -gv[4];      g2[1][1] = gv[5];      // xy (+ yx)
        g2[2][0] = -gv[5];      g2[2][1] = T(0);       // yy
        g3[0][0] = T(0);        g3[0][1] = gv[6];      // xxx
        g3[1][0] = -gv[6];      g3[1][1] = T(0);       // xxy: (0,0,1) of channel x
        g3[2][0] = T(0);        g3[2][1] = gv[6];      // xyy: (1,1,0) of channel y
        g3[3][0] = -gv[6];      g3[3][1] = T(0);       // yyy
    }
    // the incoming gradient gout [M][2] = (g_d, g_r) of a vorticity residual (MASK = ORDV_AS), its coefficients and the
    // forward's aux[m][0..3] = (u_x_b, u_y_b, w_x_b, w_y_b), as the gradient that arrives at the seven vorticity terms:
    //   d r / d (u_x, u_y) = dt tau (w_x_b, w_y_b),  d div_b / d div = tau,  d r / d w = time_term,
    //   d r / d (w_x, w_y) = dt tau (u_x_b, u_y_b),  d r / d lap w = -dt nu tau
    __device__ __forceinline__ void load_vorticity_residual(int64_t m, const T* __restrict__ GR, const VortResid<T>& vz) {
        const T gd = GR[m * 2], gr = GR[m * 2 + 1];
        const T tau = vz.tau_pt ? vz.tau_pt[m] : vz.tau;
        T ax[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ax[q] = vz.aux ? vz.aux[m * 4 + q] : T(0);
        const T k = gr * vz.dt * tau;
        T gv[NVORT];
        gv[0] = k * ax[2];      gv[1] = k * ax[3];
        gv[2] = gd * tau;       gv[3] = gr * vz.time_term;
        gv[4] = k * ax[0];      gv[5] = k * ax[1];
        gv[6] = -k * vz.nu;
        form_vorticity(gv);
    }
    // the same for the vorticity fit's gout [M][3] = (g_d, g_r, g_f): w also receives g_f data_weight.  (Written out a
    // second time: with the body shared, the ORDN backward kernels no longer compiled to the instructions they had.)
    __device__ __forceinline__ void load_vorticity_fit(int64_t m, const T* __restrict__ GR, const VortFit<T>& vz) {
        const T gd = GR[m * 3], gr = GR[m * 3 + 1], gf = GR[m * 3 + 2];
        const T tau = vz.tau_pt ? vz.tau_pt[m] : vz.tau;
        T ax[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ax[q] = vz.aux ? vz.aux[m * 4 + q] : T(0);
        const T k = gr * vz.dt * tau;
        T gv[NVORT];
        gv[0] = k * ax[2];      gv[1] = k * ax[3];
        gv[2] = gd * tau;       gv[3] = fma_<T>(gf, vz.data_weight, gr * vz.time_term);
        gv[4] = k * ax[0];      gv[5] = k * ax[1];
        gv[6] = -k * vz.nu;
        form_vorticity(gv);
    }
    // the incoming gradient gr [M][c] of a general residual (MASK = ORDR_AS), its coefficients k at the point and the
    // forward's aux (u, d_i u; read when `advects`)
    __device__ __forceinline__ void form_terms(const T* gr, const TermsAt<T, D>& k, bool advects, const T* u, const T* du,
                                               const Terms<T>& tz) {
        static_assert(MASK == ORDR_AS, "a residual's backward runs on orders 0, 1 and the trace");
        T coef[D];      // a1_i + adv w_i
#pragma unroll
        for (int i = 0; i < D; ++i) coef[i] = k.a1[i];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) g0[ch] = k.a0 * gr[ch];
        if (advects) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                T w = T(0), dot = T(0);      // w_i and sum_ch gr_ch d_i u_ch
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    w = fma_<T>(tz.B[i][ch], u[ch], w);
                    dot = fma_<T>(gr[ch], du[i * C + ch], dot);
                }
                coef[i] = fma_<T>(k.adv, w, coef[i]);
                dot *= k.adv;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) g0[ch] = fma_<T>(tz.B[i][ch], dot, g0[ch]);
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
#pragma unroll
            for (int i = 0; i < D; ++i) g1[i][ch] = coef[i] * gr[ch];
#pragma unroll
            for (int kk = 0; kk < Sym<D>::NF; ++kk) g2[kk][ch] = (kk == 0 || kk == Sym<D>::NF - 1) ? k.aL * gr[ch] : T(0);
        }
    }
    // the same with everything read at point m (lane = point)
    __device__ __forceinline__ void load_terms(int64_t m, const T* __restrict__ GR, const Terms<T>& tz) {
        TermsAt<T, D> k;
        k.load(tz, m);
        T gr[C], ax[(1 + D) * C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) gr[ch] = GR[m * C + ch];
#pragma unroll
        for (int q = 0; q < (1 + D) * C; ++q) ax[q] = tz.aux ? tz.aux[m * (1 + D) * C + q] : T(0);
        form_terms(gr, k, tz.aux != nullptr, ax, ax + C, tz);
    }
};

// Flat backward accumulator: [g_means D][g_conics NF][g_values C]
template <int D, int C> struct BwdLayout {
    static constexpr int MU = 0;
    static constexpr int CON = D;
    static constexpr int VAL = D + Sym<D>::NF;
    static constexpr int N = D + Sym<D>::NF + C;
};

// FAR_GUARD (the dense kernels, which meet every pair, and the binned third-derivative backward,
// whose waves evaluate a queued Gaussian for all 64 points of the cell): where g has underflowed
// to zero the polynomial factors can overflow (p^4 C ~ 1e38 for sigma ~ 1e-4 of the distance)
// and 0 * inf would poison the sums; such a pair contributes exactly nothing, so its x and p are
// zeroed (v_exp_f32 flushes denormals: g is either above 1e-38 or exactly 0).
//
// FACTORED (D = 2, C = 1 only): what depends on the Gaussian alone is left out of the per-pair work
// and applied once per Gaussian by the caller (plan_unpermute_kernel):
//   acc[MU]  = sum_m g (A x - dA)                    -> dL/dmu = v C acc[MU]      (A p - C dA = C (A x - dA))
//   acc[CON] = sum_m g (-A x x^T / 2 + dA x^T + E)   -> dL/dC  = v acc[CON]
//   acc[VAL] = sum_m g F                             (unchanged)
// 38 instead of 46 instructions per pair for orders 0..2.
template <typename T, int D, int C, int MASK, bool FAR_GUARD = false, bool FACTORED = false>
__device__ __forceinline__ void bwd_accumulate(T* acc, const T* s, const T* mu, const T* con, const T* v,
                                               const Gsym<T, D, C, MASK>& G) {
    static_assert(!FACTORED || (D == 2 && C == 1), "the factored form is written for d = 2, c = 1");
    using L = BwdLayout<D, C>;
    Pair<T, D> pr;
    pr.eval(s, mu, con);
    const T g = pr.g;
    if constexpr (FAR_GUARD) {
        const bool live = g > T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            pr.p[i] = live ? pr.p[i] : T(0);
            pr.x[i] = live ? pr.x[i] : T(0);
        }
    }
    if constexpr (D == 1) {
        const T p = pr.p[0], x = pr.x[0], a = con[0];
        const T t2 = fma_<T>(p, p, -a);        // p^2 - a
        const T t3 = p * (T(2) * a - t2);      // 3 a p - p^3
        T A = 0, dA = 0, E = 0;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            T F = 0, dF = 0, eF = 0;
            if constexpr ((MASK & ORD0) != 0) F += G.g0[ch];
            if constexpr ((MASK & ORD1) != 0) { F = fma_<T>(-G.g1[0][ch], p, F); dF -= G.g1[0][ch]; }
            if constexpr ((MASK & (ORD2 | ORD2T)) != 0) {
                F = fma_<T>(G.g2[0][ch], t2, F);
                dF = fma_<T>(T(2) * G.g2[0][ch], p, dF);
                eF -= G.g2[0][ch];
            }
            if constexpr ((MASK & ORD3) != 0) {
                F = fma_<T>(G.g3[0][ch], t3, F);
                dF = fma_<T>(G.g3[0][ch], T(-3) * t2, dF);     // d/dp (3ap - p^3) = 3a - 3p^2
                eF = fma_<T>(T(3) * G.g3[0][ch], p, eF);       // d/da (3ap) = 3p
            }
            acc[L::VAL + ch] = fma_<T>(g, F, acc[L::VAL + ch]);
            A = fma_<T>(v[ch], F, A);
            dA = fma_<T>(v[ch], dF, dA);
            E = fma_<T>(v[ch], eF, E);
        }
        acc[L::MU] = fma_<T>(g, fma_<T>(A, p, -dA * a), acc[L::MU]);
        acc[L::CON] = fma_<T>(g, fma_<T>(T(-0.5) * A * x, x, fma_<T>(dA, x, E)), acc[L::CON]);
    } else {
        const T px = pr.p[0], py = pr.p[1], dx = pr.x[0], dy = pr.x[1];
        const T a = con[0], b = con[1], c = con[2];
        const T txx = fma_<T>(px, px, -a), txy = fma_<T>(px, py, -b), tyy = fma_<T>(py, py, -c);
        T A = 0, dAx = 0, dAy = 0, Exx = 0, Exy = 0, Eyy = 0;   // Exy holds E_01 + E_10
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            T F = 0, dFx = 0, dFy = 0, exx = 0, exy = 0, eyy = 0;
            if constexpr ((MASK & ORD0) != 0) F += G.g0[ch];
            if constexpr ((MASK & ORD1) != 0) {
                F = fma_<T>(-G.g1[0][ch], px, F);
                F = fma_<T>(-G.g1[1][ch], py, F);
                dFx -= G.g1[0][ch];
                dFy -= G.g1[1][ch];
            }
            if constexpr ((MASK & (ORD2 | ORD2T)) != 0) {
                const T hxx = G.g2[0][ch], hxy = G.g2[1][ch], hyy = G.g2[2][ch];
                F = fma_<T>(hxx, txx, F);
                F = fma_<T>(hxy, txy, F);
                F = fma_<T>(hyy, tyy, F);
                dFx = fma_<T>(T(2) * hxx, px, fma_<T>(hxy, py, dFx));
                dFy = fma_<T>(T(2) * hyy, py, fma_<T>(hxy, px, dFy));
                exx -= hxx;
                exy -= hxy;
                eyy -= hyy;
            }
            if constexpr ((MASK & ORD3) != 0) {
                const T k0 = G.g3[0][ch], k1 = G.g3[1][ch], k2 = G.g3[2][ch], k3 = G.g3[3][ch];
                // poly: xxx = 3a px - px^3 ; xxy = 2b px + a py - px^2 py ;
                //       xyy = c px + 2b py - px py^2 ; yyy = 3c py - py^3
                F = fma_<T>(k0, px * (T(2) * a - txx), F);
                F = fma_<T>(k1, fma_<T>(T(2) * b, px, -txx * py), F);
                F = fma_<T>(k2, fma_<T>(T(2) * b, py, -tyy * px), F);
                F = fma_<T>(k3, py * (T(2) * c - tyy), F);
                // d/dpx
                dFx = fma_<T>(k0, T(-3) * txx, dFx);
                dFx = fma_<T>(k1, T(-2) * txy, dFx);
                dFx = fma_<T>(k2, -tyy, dFx);
                // d/dpy
                dFy = fma_<T>(k1, -txx, dFy);
                dFy = fma_<T>(k2, T(-2) * txy, dFy);
                dFy = fma_<T>(k3, T(-3) * tyy, dFy);
                // explicit d/da, d/db (flat: both off-diagonal entries), d/dc
                exx = fma_<T>(T(3) * k0, px, fma_<T>(k1, py, exx));
                exy = fma_<T>(T(2) * k1, px, fma_<T>(T(2) * k2, py, exy));
                eyy = fma_<T>(T(3) * k3, py, fma_<T>(k2, px, eyy));
            }
            acc[L::VAL + ch] = fma_<T>(g, F, acc[L::VAL + ch]);
            if constexpr (C == 1) {
                // one channel: v factors out of A, dA and E -- carry it in the weight instead
                A = F; dAx = dFx; dAy = dFy; Exx = exx; Exy = exy; Eyy = eyy;
            } else {
                A = fma_<T>(v[ch], F, A);
                dAx = fma_<T>(v[ch], dFx, dAx);
                dAy = fma_<T>(v[ch], dFy, dAy);
                Exx = fma_<T>(v[ch], exx, Exx);
                Exy = fma_<T>(v[ch], exy, Exy);
                Eyy = fma_<T>(v[ch], eyy, Eyy);
            }
        }
        if constexpr (FACTORED) {
            // r = -A x / 2;  A x - dA = -(2 r + dA);  conic terms: x_k (r_k + dA_k) + E_kk, and for the
            // off-diagonal x_1 (2 r_0 + dA_0) + dA_1 x_0 + E_01 = -x_1 mx + dA_1 x_0 + E_01
            const T hA = T(-0.5) * A;
            const T rx = hA * dx, ry = hA * dy;
            const T mx = fma_<T>(T(-2), rx, -dAx), my = fma_<T>(T(-2), ry, -dAy);
            acc[L::MU + 0] = fma_<T>(g, mx, acc[L::MU + 0]);
            acc[L::MU + 1] = fma_<T>(g, my, acc[L::MU + 1]);
            acc[L::CON + 0] = fma_<T>(g, fma_<T>(rx + dAx, dx, Exx), acc[L::CON + 0]);
            acc[L::CON + 1] = fma_<T>(g, fma_<T>(-mx, dy, fma_<T>(dAy, dx, Exy)), acc[L::CON + 1]);
            acc[L::CON + 2] = fma_<T>(g, fma_<T>(ry + dAy, dy, Eyy), acc[L::CON + 2]);
            return;
        }
        const T g_ = g;
        const T g = (C == 1) ? g_ * v[0] : g_;          // weight of the mean / conic terms
        // means: g (A p_l - (dA . C)_l)
        acc[L::MU + 0] = fma_<T>(g, fma_<T>(A, px, -fma_<T>(dAx, a, dAy * b)), acc[L::MU + 0]);
        acc[L::MU + 1] = fma_<T>(g, fma_<T>(A, py, -fma_<T>(dAx, b, dAy * c)), acc[L::MU + 1]);
        // flat conic: [G00, G01 + G10, G11]
        const T hA = T(-0.5) * A;
        acc[L::CON + 0] = fma_<T>(g, fma_<T>(hA * dx, dx, fma_<T>(dAx, dx, Exx)), acc[L::CON + 0]);
        acc[L::CON + 1] = fma_<T>(g, fma_<T>(-A * dx, dy, fma_<T>(dAx, dy, fma_<T>(dAy, dx, Exy))), acc[L::CON + 1]);
        acc[L::CON + 2] = fma_<T>(g, fma_<T>(hA * dy, dy, fma_<T>(dAy, dy, Eyy)), acc[L::CON + 2]);
    }
}

}  // namespace pigs
