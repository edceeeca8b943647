// mir_kernels.hip.h -- the MIR separation of include/mipx_mir.h: one cut from one point, one box and one base row.
//
//   mir_separate  one workgroup of 256 threads (4 waves) per (point, base row).  g' and t* of the n + m <= 2048
//                 extended columns and their flags live in LDS (about 35 KiB).  Set-up: one wave per row with a
//                 nonzero multiplier sums A_i x* for the slack's value (lanes stride the columns: coalesced); one
//                 thread per column sums lambda' A over the rows (neighbouring threads read neighbouring a_ij:
//                 coalesced; with the unit rows that is one row read).  A workgroup maximum gives G, beside which an
//                 integral column's |g| may be noise.  Wave 0 builds the divisor list in column
//                 order from ballots, the list itself in its lanes' registers.  A trial is one sweep of every thread
//                 over its columns, a butterfly inside each wave and the four waves' sums through LDS; its result is
//                 the same in every thread, so the search over the divisors needs no broadcast.  Each sign's winning
//                 mu then overwrites t*, and one thread per column walks the rows once more for pi.  No atomics; the
//                 outputs are plain vector stores.
//
// Products are not fused (the library is built with -ffp-contract=off); every sum runs in the order mipx_mir.h
// states, which tests/support/mir_reference.py follows bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mipx {

constexpr int kMirNT = 256;               // threads per workgroup
constexpr int kMirMax = 1024;             // rows and columns at most
constexpr int kMirCols = 2 * kMirMax;     // extended columns at most
constexpr int kMirMaxDiv = 64;            // divisor candidates from the columns at most (one per lane of wave 0)
constexpr double kMirInside = 1e-6;       // a divisor's column is this far inside its box
constexpr double kMirTiny = 1e-9;         // an integral column with |g| at most this times the largest |g| counts as continuous

enum MirFlag : uint8_t { kMirPart = 1, kMirInt = 2, kMirComp = 4, kMirElig = 8 };

struct MirArgs {
    int m, n, n_int, R, max_div;
    double f0_min, min_eff, max_dyn;
    const double *A, *b;              // the problem's rows A x >= b (m x n, row-major)
    const double *x, *l, *u;          // batch x n
    const int32_t *int_idx;           // the integer columns, n_int of them
    const uint8_t *row_int;           // nullable: m flags, slack i is integral
    const double *mult;               // nullable: R x m multipliers (null: the m unit rows)
    double *pi, *pi0, *eff, *delta;   // batch x R x n, batch x R each
    int32_t *sign, *status;           // batch x R
};

__device__ inline double mir_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// BLOCK SUM of two values at once: the butterfly, then the waves in order.  Called by every thread.
__device__ inline void mir_block_sum2(double &a, double &b, double (*red)[kMirNT / 64]) {
    a = mir_wave_sum(a);
    b = mir_wave_sum(b);
    __syncthreads();   // (the slots may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

// The largest of a value over the workgroup (no order to state: max is exact).  Called by every thread.
__device__ inline double mir_block_max(double v, double (*red)[kMirNT / 64]) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
}

// k_j of a trial: the MIR coefficient of column j in t-space
__device__ inline double mir_coef(uint8_t flag, double gpj, double delta, double f0, double omf) {
    if (!(flag & kMirPart)) return 0.0;
    if (flag & kMirInt) {
        const double a = gpj / delta, fa = floor(a), f = a - fa, r = f - f0;
        return fa + (r > 0.0 ? r : 0.0) / omf;
    }
    return gpj < 0.0 ? gpj / (delta * omf) : 0.0;
}

__global__ void __launch_bounds__(kMirNT) mir_separate(MirArgs a) {
    __shared__ double gp[kMirCols], ts[kMirCols];
    __shared__ uint8_t fl[kMirCols];
    __shared__ double cand[kMirMaxDiv + 1];
    __shared__ double red[2][kMirNT / 64];
    __shared__ int32_t ncand, sskip;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.m, n = a.n, N = a.n + a.m;
    const size_t blk = blockIdx.x;
    const int r = (int)(blk % (size_t)a.R);
    const size_t pt = blk / (size_t)a.R;
    const double *x = a.x + pt * n, *l = a.l + pt * n, *u = a.u + pt * n;
    const double *lam = a.mult ? a.mult + (size_t)r * m : nullptr;
    const double inf = __builtin_huge_val();

    // flags of the structural columns, the slack columns at rest
    for (int j = tid; j < n; j += kMirNT) fl[j] = 0;
    for (int i = tid; i < m; i += kMirNT) { gp[n + i] = 0.0; ts[n + i] = 0.0; fl[n + i] = 0; }
    if (tid == 0) sskip = 0;
    __syncthreads();
    for (int k = tid; k < a.n_int; k += kMirNT) fl[a.int_idx[k]] = kMirInt;
    // slack columns of the rows with a multiplier: s*_i from a wave sum of A_i x*
    for (int i = wave; i < m; i += kMirNT / 64) {
        const double li = lam ? lam[i] : (i == r ? 1.0 : 0.0);
        if (li == 0.0) continue;   // (uniform over the wave)
        const double *ar = a.A + (size_t)i * n;
        double s = 0.0;
        for (int j = lane; j < n; j += 64) s += ar[j] * x[j];
        s = mir_wave_sum(s);
        if (lane == 0) {
            const double sv = s - a.b[i], st = sv > 0.0 ? sv : 0.0;
            const bool isint = a.row_int && a.row_int[i];
            gp[n + i] = 0.0 - li;
            ts[n + i] = st;
            fl[n + i] = (uint8_t)(kMirPart | (isint ? kMirInt : 0) | (isint && st > kMirInside ? kMirElig : 0));
        }
    }
    // d0 = lambda' b, the same in every thread
    double d0 = 0.0;
    if (lam) {
        for (int i = 0; i < m; i++) {
            const double li = lam[i];
            if (li != 0.0) d0 += li * a.b[i];
        }
    } else {
        d0 += 1.0 * a.b[r];
    }
    __syncthreads();   // (the integer flags are in place)
    // structural columns: lambda' A, the substitution, the constant K
    double kpart = 0.0, zero = 0.0;
    for (int j = tid; j < n; j += kMirNT) {
        double g = 0.0;
        if (lam) {
            for (int i = 0; i < m; i++) {
                const double li = lam[i];
                if (li != 0.0) g += li * a.A[(size_t)i * n + j];
            }
        } else {
            g += 1.0 * a.A[(size_t)r * n + j];
        }
        const double xj = x[j], lj = l[j], uj = u[j];
        const bool comp = uj < inf && (uj - xj < xj - lj);
        const double tj = comp ? uj - xj : xj - lj, bnd = comp ? uj : lj;
        const bool part = g != 0.0, isint = (fl[j] & kMirInt) != 0;
        const bool elig = part && isint && tj > kMirInside && (!(uj < inf) || (uj - lj) - tj > kMirInside);
        if (part && isint && floor(bnd) != bnd) sskip = 1;
        gp[j] = comp ? 0.0 - g : g;
        ts[j] = tj;
        fl[j] = (uint8_t)((part ? kMirPart : 0) | (isint ? kMirInt : 0) | (comp ? kMirComp : 0) | (elig ? kMirElig : 0));
        kpart += g * bnd;
    }
    mir_block_sum2(kpart, zero, red);   // (its barriers also publish gp, ts, fl and sskip)
    const double dp = d0 - kpart;       // d' of the sign +1; that of -1 is its negative, bit for bit, as g' is
    const bool skipped = sskip != 0;
    // G, the largest |g|; an integral column whose |g| is noise beside it is rounded as a continuous one
    double gmax = 0.0;
    for (int j = tid; j < N; j += kMirNT) gmax = fmax(gmax, fabs(gp[j]));
    const double G = mir_block_max(gmax, red);
    for (int j = tid; j < N; j += kMirNT)
        if ((fl[j] & kMirInt) && fabs(gp[j]) <= kMirTiny * G) fl[j] &= (uint8_t)~(kMirInt | kMirElig);
    __syncthreads();

    // the divisor list, in column order: lane k of wave 0 holds candidate k
    if (wave == 0) {
        double mine = 0.0;
        int nc = 0;
        for (int base = 0; base < N && nc < a.max_div; base += 64) {
            const int j = base + lane;
            unsigned long long mask = __ballot(j < N && (fl[j] & kMirElig));
            while (mask && nc < a.max_div) {
                const int q = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const double v = fabs(gp[base + q]);
                if (!__any(lane < nc && mine == v)) {
                    if (lane == nc) mine = v;
                    nc++;
                }
            }
        }
        const bool has1 = __any(lane < nc && mine == 1.0);
        if (lane < nc) cand[lane] = mine;
        if (lane == 0) {
            if (!has1) cand[nc] = 1.0;
            ncand = has1 ? nc : nc + 1;
        }
    }
    __syncthreads();
    const int nc = ncand;

    // the trials: every thread ends each of them with the same efficacy, so each sign's winner is known to all
    bool shave[2] = {false, false};
    double sdelta[2] = {0.0, 0.0};
    if (!skipped) {
        for (int s = 0; s < 2; s++) {
            const double sg = s ? -1.0 : 1.0;
            double seff = 0.0, star = 0.0;
            for (int k = 0; k < nc + 3; k++) {
                if (k == nc) {
                    if (!shave[s]) break;
                    star = sdelta[s];
                }
                const double delta = k < nc ? cand[k] : star / (double)(2 << (k - nc));
                const double beta = (sg * dp) / delta, flb = floor(beta), f0 = beta - flb;
                if (!(G / delta <= a.max_dyn && fabs(beta) <= a.max_dyn)) continue;
                if (!(f0 >= a.f0_min && f0 <= 1.0 - a.f0_min)) continue;
                const double omf = 1.0 - f0;
                double P = 0.0, Q = 0.0;
                for (int j = tid; j < N; j += kMirNT) {
                    const double kj = mir_coef(fl[j], sg * gp[j], delta, f0, omf);
                    P += kj * ts[j];
                    Q += kj * kj;
                }
                mir_block_sum2(P, Q, red);
                if (!(Q > 0.0)) continue;
                const double eff = (P - flb) / sqrt(Q);
                if (!(eff - eff == 0.0)) continue;   // (not finite)
                if (!shave[s] || eff > seff) { shave[s] = true; seff = eff; sdelta[s] = delta; }
            }
        }
    }

    double *pi = a.pi + blk * n;
    if (!shave[0] && !shave[1]) {
        for (int j = tid; j < n; j += kMirNT) pi[j] = 0.0;
        if (tid == 0) {
            a.pi0[blk] = 0.0; a.eff[blk] = 0.0; a.delta[blk] = 0.0; a.sign[blk] = 0;
            a.status[blk] = skipped ? 4 : 1;
        }
        return;
    }
    // each sign's winner as a cut in x: mu over t* (no trial follows), nu, then pi and pi0 through s = A x - b; the
    // sign with the larger x-space efficacy is written, +1 on a tie
    bool have = false;
    double w_eff = 0.0;
    for (int s = 0; s < 2; s++) {
        if (!shave[s]) continue;   // (uniform)
        const double sg = s ? -1.0 : 1.0, delta = sdelta[s];
        const double beta = (sg * dp) / delta, flb = floor(beta), f0 = beta - flb, omf = 1.0 - f0;
        double C = 0.0;
        zero = 0.0;
        for (int j = tid; j < N; j += kMirNT) {
            const uint8_t f = fl[j];
            const double kj = mir_coef(f, sg * gp[j], delta, f0, omf);
            const bool comp = (f & kMirComp) != 0;
            const double lj = j < n ? l[j] : 0.0;
            C += comp ? 0.0 - kj * u[j] : kj * lj;   // (a complemented column is structural)
            ts[j] = comp ? 0.0 - kj : kj;
        }
        mir_block_sum2(C, zero, red);   // (its barriers publish mu)
        const double nu = flb + C;
        double acc0 = nu;
        for (int i = 0; i < m; i++) {
            const double ms = ts[n + i];
            if (ms != 0.0) acc0 += ms * a.b[i];
        }
        const double pi0 = 0.0 - acc0;
        double V = 0.0, W = 0.0, mx = 0.0, mn = inf;
        double pj[kMirMax / kMirNT];
#pragma unroll
        for (int c = 0; c < kMirMax / kMirNT; c++) {
            const int j = tid + c * kMirNT;
            pj[c] = 0.0;
            if (j >= n) continue;
            double acc = ts[j];
            for (int i = 0; i < m; i++) {
                const double ms = ts[n + i];
                if (ms != 0.0) acc += ms * a.A[(size_t)i * n + j];
            }
            pj[c] = 0.0 - acc;
            const double ap = fabs(pj[c]);
            V += pj[c] * x[j];
            W += pj[c] * pj[c];
            if (ap > mx) mx = ap;
            if (ap != 0.0 && ap < mn) mn = ap;
        }
        mir_block_sum2(V, W, red);   // (behind its barriers nobody reads this sign's mu any more)
        const double effx = W > 0.0 ? (pi0 - V) / sqrt(W) : 0.0;
        if (have && !(effx > w_eff)) continue;   // (uniform)
        have = true;
        w_eff = effx;
        for (int off = 32; off > 0; off >>= 1) {
            mx = fmax(mx, __shfl_xor(mx, off, 64));
            mn = fmin(mn, __shfl_xor(mn, off, 64));
        }
        __syncthreads();
        if (lane == 0) { red[0][wave] = mx; red[1][wave] = mn; }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kMirMax / kMirNT; c++) {
            const int j = tid + c * kMirNT;
            if (j < n) pi[j] = pj[c];
        }
        if (tid == 0) {
            for (int w = 0; w < kMirNT / 64; w++) { mx = fmax(mx, red[0][w]); mn = fmin(mn, red[1][w]); }
            int status = 0;
            if (!(effx > a.min_eff)) status = 2;
            else if (mx / mn > a.max_dyn) status = 3;
            a.pi0[blk] = pi0; a.eff[blk] = effx; a.delta[blk] = delta; a.sign[blk] = s ? -1 : 1;
            a.status[blk] = status;
        }
    }
}

}  // namespace mipx
