// One TDOA task on one wavefront: the ONE statement of the estimator's arithmetic (reference
// thrifty/tdoa_est.py:58-71, 89-222; thrifty/stat_tools.py:8-41), shared by tdoa.hip (a task's list is its
// receiver pair's beacon pairs) and tdoamatrix.hip (a task's list is ONE beacon's rows at its receiver pair).
//   Python's two bisections on the list's det0 timestamps (sorted or not), the median / MAD outlier mask on
//   soa0 - soa1 in the reference's float64 operations, the MODEL over the kept pairs -- a least-squares
//   polynomial of soa0 on soa1 + beacon_sdoa (plain or weighted), the nearest kept pair, or the line through
//   two kept pairs of one beacon -- and the |tdoa| >= MAX_TDOA failure.
// A task finds its list through a LIST type:
//   const double *ts, *soa0, *soa1, *q0, *q1   the list's columns, n entries (det0 timestamp, the two SoAs, the
//   int n                                      two (energy / noise)**2)
//   int beacon(int i) const                    which beacon entry i is of (compared for equality only)
//   double beacon_tdoa(int i) const            (dist(rx0, beacon) - dist(rx1, beacon)) / c of entry i
// The fit is not LAPACK's: it runs in u = (x - mean) / max|x - mean| on y - mean(y) (normal equations of
// size deg + 1, partial pivoting, Horner in u), which keeps the digits the raw Vandermonde of abscissae
// near 1e9..1e11 loses.  Everything that decides WHICH pairs are used is the reference's arithmetic.
// The nearest and the linear model bisect the KEPT list (the window's pairs the mask left, in list order):
// kept rank -> window position goes through per-trip ballots and popcounts (kept_at), whatever the window's
// length; their formulas are the reference's operations in its order, so their results are its bits.
//
// Everything here is a template or inline: both files include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/thrifty_hip.h"

// the outlier mask must equal numpy's bit for bit: no a * b + c may become an fma in a file that includes
// this (the build also passes -ffp-contract=off to both, thrifty_amd/build.py: PER_FILE_FLAGS)
#pragma clang fp contract(off)

namespace thr {
namespace tdoa_task {

constexpr int kBlock = 256;               // workgroup size of the estimate kernels
constexpr int kWave = 64;                 // one task per wavefront
constexpr int kWaves = kBlock / kWave;    // tasks per workgroup (_native.TDOA_TASKS_PER_WORKGROUP)
constexpr int kLdsWindow = 256;           // windows up to this many pairs are staged in LDS (_native.TDOA_LDS_WINDOW)
constexpr double kSpeedOfLight = 2.997e8;           // the reference's constant (tdoa_est.py:25)
constexpr double kMaxTdoa = 30e3 / kSpeedOfLight;   // tdoa_est.py:26

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);  // commutative: every lane the same bits
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, kWave));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
// the value of the one lane that holds it (`mine`), unchanged bits; 0 if no lane does (NaN input)
__device__ __forceinline__ double wave_pick(double v, bool mine) {
    const unsigned long long who = __ballot(mine);
    if (who == 0) return 0.0;
    return __shfl(v, __ffsll((long long)who) - 1, kWave);
}
// LDS written by some lanes of this wavefront, read by others: order the accesses, nothing more (the
// wavefronts of a workgroup run different tasks and never meet at a workgroup barrier)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The window of one task: pairs [0, n) of a bucket.  value(i) is sdoa_i = soa0 - soa1 (deviation ==
// false) or sqrt((sdoa_i - median)**2) (deviation == true), from LDS when the window was staged there
// and recomputed from the columns otherwise -- the same float64 operations either way.
struct Window {
    const double* soa0;
    const double* soa1;
    const double* lds;  // null: not staged
    int n;
    bool deviation;
    double median;
    __device__ __forceinline__ double compute(int i) const {
        double v = soa0[i] - soa1[i];
        if (deviation) {
            const double c = v - median;
            v = __dsqrt_rn(c * c);
        }
        return v;
    }
    __device__ __forceinline__ double value(int i) const { return lds ? lds[i] : compute(i); }
};
// np.median: the element of rank (n - 1) / 2, or the mean of the two middle ones.  Every element's rank
// is counted against all others (ties broken by position, so the ranks are a permutation): exact for
// every n; lanes stride over the elements, so a window longer than a wavefront takes several trips.
__device__ inline double wave_median(const Window& w, int lane) {
    const int r_lo = (w.n - 1) / 2, r_hi = w.n / 2;
    double v_lo = 0.0, v_hi = 0.0;
    bool has_lo = false, has_hi = false;
    for (int i = lane; i < w.n; i += kWave) {
        const double v = w.value(i);
        int rank = 0;
        for (int j = 0; j < w.n; ++j) {
            const double o = w.value(j);
            rank += (o < v || (o == v && j < i)) ? 1 : 0;
        }
        if (rank == r_lo) {
            v_lo = v;
            has_lo = true;
        }
        if (rank == r_hi) {
            v_hi = v;
            has_hi = true;
        }
    }
    v_lo = wave_pick(v_lo, has_lo);
    if (r_lo == r_hi) return v_lo;
    v_hi = wave_pick(v_hi, has_hi);
    return (v_lo + v_hi) / 2.0;
}

struct Estimate {      // what a task leaves, the same in every lane
    bool good;         // a TDOA inside the range
    bool modelled;     // the model gave a value (good or out of range)
    double tdoa, quality;
    int n_window, n_kept;
    int pick0, pick1;  // positions in the kept list: {idx, -1} (nearest), {low, high} (linear)
};

// The task (t0, soa_d0, soa_d1: the det0 timestamp and the two SoAs of its detection pair) on list L; `lds`
// is this wavefront's kLdsWindow doubles.  Every lane of the wavefront calls it.
template <int DEG, int MODEL, class List>
__device__ __forceinline__ Estimate estimate(const List& L, double t0, double soa_d0, double soa_d1, double window,
                                             double sample_rate, int lane, double* lds_wave) {
    constexpr int M = DEG + 1;
    constexpr bool kFit = MODEL == THR_TDOA_POLY || MODEL == THR_TDOA_WEIGHTED_POLY;  // DEG is read by these only
    constexpr bool kWeighted = MODEL == THR_TDOA_WEIGHTED_POLY;
    constexpr int kMinKept = MODEL == THR_TDOA_NEAREST ? 1 : MODEL == THR_TDOA_LINEAR ? 2 : M;
    const int n_list = L.n;
    const double* list_ts = L.ts;

    // bisect_left(list, t0 - window), bisect_right(list, t0 + window): Python's loops, whatever the order
    // of the list (every lane runs them; the loads are one address per wavefront)
    const double start = t0 - window, stop = t0 + window;
    int lo = 0, hi = n_list;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (list_ts[mid] < start)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int left = lo;
    lo = 0, hi = n_list;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (stop < list_ts[mid])
            hi = mid;
        else
            lo = mid + 1;
    }
    const int n_window = lo > left ? lo - left : 0;
    const double* w_soa0 = L.soa0 + left;
    const double* w_soa1 = L.soa1 + left;
    const double* w_q0 = L.q0 + left;
    const double* w_q1 = L.q1 + left;

    // is_outlier(sdoa) if the window holds more than one pair: dropped where 0.6745 * diff / mad > 3.5
    // (mad == 0: 0 / 0 is NaN and stays, x / 0 is inf and goes)
    const bool masked = n_window > 1;
    double* lds = n_window <= kLdsWindow ? lds_wave : nullptr;
    Window w{w_soa0, w_soa1, nullptr, n_window, false, 0.0};
    double mad = 0.0;
    if (masked) {
        if (lds) {
            for (int i = lane; i < n_window; i += kWave) lds[i] = w.compute(i);
            wave_sync();
            w.lds = lds;
        }
        w.median = wave_median(w, lane);
        w.deviation = true;
        if (lds) {
            wave_sync();  // every rank is counted before the values are replaced
            for (int i = lane; i < n_window; i += kWave) lds[i] = w.compute(i);
            wave_sync();
        }
        mad = wave_median(w, lane);
    }
    auto kept = [&](int i) { return !masked || !(0.6745 * w.value(i) / mad > 3.5); };
    // x = soa1 + beacon_sdoa, beacon_sdoa = (dist(rx0, b) - dist(rx1, b)) / c * sample_rate; y = soa0
    auto abscissa = [&](int i) {
        const double tdoa = L.beacon_tdoa(left + i);
        return w_soa1[i] + tdoa * sample_rate;
    };
    // beacon_sdoa alone, the same operations
    auto beacon_sdoa = [&](int i) {
        const double tdoa = L.beacon_tdoa(left + i);
        return tdoa * sample_rate;
    };
    // window position of the kept pair of rank `rank` (0 <= rank < n_kept, the same in every lane): per trip
    // of 64 positions a ballot of the kept ones; the trip that holds the rank names the lane by its prefix count
    auto kept_at = [&](int rank) {
        int before = 0;
        for (int base = 0; base < n_window; base += kWave) {
            const int i = base + lane;
            const bool mine = i < n_window && kept(i);
            const unsigned long long set = __ballot(mine);
            const int here = __popcll(set);
            if (rank < before + here) {
                const int prefix = __popcll(set & ((1ull << lane) - 1ull));
                const unsigned long long hit = __ballot(mine && prefix == rank - before);
                return base + __ffsll((long long)hit) - 1;
            }
            before += here;
        }
        return 0;  // not reached for a rank below n_kept
    };
    // bisect_left(T, t0) over the kept pairs' det0 timestamps: Python's probes, in kept coordinates
    auto bisect_kept = [&](int n_kept_) {
        int a = 0, b = n_kept_;
        while (a < b) {
            const int mid = (a + b) / 2;
            if (list_ts[left + kept_at(mid)] < t0)
                a = mid + 1;
            else
                b = mid;
        }
        return a;
    };

    // pass 1: how many are kept, the means, model_quality
    int n_kept = 0;
    double sum_x = 0.0, sum_y = 0.0, sum_q0 = 0.0, sum_q1 = 0.0;
    for (int i = lane; i < n_window; i += kWave)
        if (kept(i)) {
            ++n_kept;
            if constexpr (kFit) {
                sum_x += abscissa(i);
                sum_y += w_soa0[i];
            }
            sum_q0 += w_q0[i];
            sum_q1 += w_q1[i];
        }
    n_kept = wave_sum(n_kept);
    bool good = n_kept >= kMinKept;
    bool modelled = false;
    double tdoa = 0.0, quality = 0.0;
    int pick0 = -1, pick1 = -1;  // positions in the kept list: {idx, -1} (nearest), {low, high} (linear)
    if constexpr (MODEL == THR_TDOA_NEAREST) {
        if (good) {
            quality = (wave_sum(sum_q0) / n_kept + wave_sum(sum_q1) / n_kept) / 2.0;
            // the kept pair whose det0 timestamp is nearest to t0; a tie stays on the later one
            int idx = bisect_kept(n_kept);
            if (idx > 0) {
                bool earlier = idx == n_kept;
                if (!earlier)
                    earlier = fabs(t0 - list_ts[left + kept_at(idx - 1)]) < fabs(t0 - list_ts[left + kept_at(idx)]);
                if (earlier) --idx;
            }
            pick0 = idx;
            const int i = kept_at(idx);
            const double dsoa0 = soa_d0 - w_soa0[i], dsoa1 = soa_d1 - w_soa1[i];
            tdoa = (dsoa0 - dsoa1 + beacon_sdoa(i)) / sample_rate;
            modelled = true;
            good = !(fabs(tdoa) >= kMaxTdoa);
        }
    } else if constexpr (MODEL == THR_TDOA_LINEAR) {
        if (good) {
            quality = (wave_sum(sum_q0) / n_kept + wave_sum(sum_q1) / n_kept) / 2.0;
            int high = bisect_kept(n_kept);
            if (high == n_kept) high = n_kept - 1;
            const int i_high = kept_at(high);
            // down the kept list to the nearest pair of the same beacon: window positions, the dropped ones skipped
            // (every lane reads the same position)
            int low = high - 1, i_low = i_high - 1;
            while (i_low >= 0 && !(kept(i_low) && L.beacon(left + i_low) == L.beacon(left + i_high))) {
                if (kept(i_low)) --low;
                --i_low;
            }
            if (i_low < 0) low = -1;
            pick0 = low;
            pick1 = high;
            good = low >= 0 && w_soa0[i_high] != w_soa0[i_low];  // equal SoAs: the reference divides by zero
            if (good) {
                const double weight = (soa_d0 - w_soa0[i_low]) / (w_soa0[i_high] - w_soa0[i_low]);
                const double tau = (w_soa1[i_low] * (1.0 - weight) + w_soa1[i_high] * weight) - soa_d1;
                tdoa = (tau + beacon_sdoa(i_high)) / sample_rate;
                modelled = true;
                good = !(fabs(tdoa) >= kMaxTdoa);
            }
        }
    } else if (good) {
        const double mean_x = wave_sum(sum_x) / n_kept, mean_y = wave_sum(sum_y) / n_kept;
        quality = (wave_sum(sum_q0) / n_kept + wave_sum(sum_q1) / n_kept) / 2.0;
        // the weighted fit: w = (sqrt(sqrt(1 / |soa0_i - soa0|) / max) + 2) / 3, numpy's float64 operations;
        // a kept pair AT the task's soa0 has no finite weight: a failure (the reference appends a NaN row)
        double raw_max = 0.0;
        auto raw_weight = [&](int i) { return __dsqrt_rn(1.0 / fabs(w_soa0[i] - soa_d0)); };
        auto weight = [&](int i) { return (__dsqrt_rn(raw_weight(i) / raw_max) + 2.0) / 3.0; };
        if constexpr (kWeighted) {
            for (int i = lane; i < n_window; i += kWave)
                if (kept(i)) raw_max = fmax(raw_max, raw_weight(i));
            raw_max = wave_max(raw_max);
            good = raw_max < INFINITY;
        }
        // pass 2: the scale, and DEG + 1 distinct abscissae (the smallest, the next larger one, ...)
        double below = -INFINITY, scale = 0.0;
        for (int k = 0; k < M && good; ++k) {
            double next = INFINITY;
            for (int i = lane; i < n_window; i += kWave)
                if (kept(i)) {
                    const double x = abscissa(i);
                    if (x > below) next = fmin(next, x);
                    if (k == 0) scale = fmax(scale, fabs(x - mean_x));
                }
            next = wave_min(next);
            good = next < INFINITY;
            below = next;
        }
        scale = wave_max(scale);
        if (good) {
            // pass 3: the moments of u = (x - mean_x) / scale in [-1, 1] against v = y - mean_y
            double s[2 * DEG + 1], t[M];
#pragma unroll
            for (int k = 0; k <= 2 * DEG; ++k) s[k] = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) t[k] = 0.0;
            for (int i = lane; i < n_window; i += kWave)
                if (kept(i)) {
                    const double u = (abscissa(i) - mean_x) / scale, v = w_soa0[i] - mean_y;
                    double p = 1.0;
                    if constexpr (kWeighted) {  // the moments carry w^2
                        const double wi = weight(i);
                        p = wi * wi;
                    }
#pragma unroll
                    for (int k = 0; k <= 2 * DEG; ++k) {
                        s[k] += p;
                        if (k < M) t[k] += p * v;
                        p *= u;
                    }
                }
#pragma unroll
            for (int k = 0; k <= 2 * DEG; ++k) s[k] = wave_sum(s[k]);
#pragma unroll
            for (int k = 0; k < M; ++k) t[k] = wave_sum(t[k]);
            // normal equations, Gaussian elimination with partial pivoting (every lane the same)
            double a[M][M + 1];
#pragma unroll
            for (int r = 0; r < M; ++r) {
#pragma unroll
                for (int c = 0; c < M; ++c) a[r][c] = s[r + c];
                a[r][M] = t[r];
            }
#pragma unroll
            for (int c = 0; c < M; ++c) {
#pragma unroll
                for (int r = c + 1; r < M; ++r)
                    if (fabs(a[r][c]) > fabs(a[c][c])) {
#pragma unroll
                        for (int k = 0; k <= M; ++k) {
                            const double swap = a[c][k];
                            a[c][k] = a[r][k];
                            a[r][k] = swap;
                        }
                    }
#pragma unroll
                for (int r = c + 1; r < M; ++r) {
                    const double f = a[r][c] / a[c][c];
#pragma unroll
                    for (int k = c; k <= M; ++k) a[r][k] -= f * a[c][k];
                }
            }
            double coef[M];
#pragma unroll
            for (int r = M - 1; r >= 0; --r) {
                double acc = a[r][M];
#pragma unroll
                for (int k = r + 1; k < M; ++k) acc -= a[r][k] * coef[k];
                coef[r] = acc / a[r][r];
            }
            // tdoa = (det0.soa - fit(det1.soa)) / sample_rate, fit(x) = mean_y + p(u(x)): the large parts
            // cancel before the small one is subtracted
            const double u = (soa_d1 - mean_x) / scale;
            double p = coef[M - 1];
#pragma unroll
            for (int k = M - 2; k >= 0; --k) p = p * u + coef[k];
            tdoa = ((soa_d0 - mean_y) - p) / sample_rate;
            modelled = true;
            good = !(fabs(tdoa) >= kMaxTdoa);
        }
    }
    return Estimate{good, modelled, tdoa, quality, n_window, n_kept, pick0, pick1};
}

}  // namespace tdoa_task
}  // namespace thr
