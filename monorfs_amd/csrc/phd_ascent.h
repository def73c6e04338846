// phd_ascent.h — the smoother's pose search resident on the device (phd_quasi_ascent): LoopyPHDNavigator.LogLikeGradientAscent
// (LoopyPHDNavigator.cs:916-965) for n initial estimates side by side, and the finite-difference Hessian rows of
// LogLikeFitCovariance (:976-1021). monorfs_amd/loopy.py::LogLikeGradientAscent is the statement of the order of operations;
// everything here is FP64 without contraction where it restates that loop.
//
// The evaluations are alpha_assoc_body's, through wrappers that differ from k_quasi_setll / k_quasi_setll_grad in one thing: a
// workgroup whose estimate has stopped returns at once. What lies between two evaluations is done by small control kernels over
// per-estimate state that never leaves the device (AscentBufs):
//   k_ascent_begin       nextpose7 = Add(lin, pose6), prev = -inf, iterations = 0
//   (gradient launch)    value and gradient at nextpose7
//   k_ascent_start       loglike = that value (:928-929); active = loglike - prev > 1e-3
//   per iteration:       (gradient launch at nextpose7 — iteration 0 keeps the first launch's: same pose, same kernel, same bits)
//   k_ascent_candidates  clip, the 16 halved steps, their poses
//   (value launch)       the 16 candidates of every active estimate
//   k_ascent_select      the do-while of :943-951, the gain test, the count of estimates still active
//   k_ascent_hess_poses, (gradient launch), k_ascent_hess_rows: the 12 poses pose6 +- 1e-5 e_i and the central differences
// Every evaluation launch finds the batch's slab counter at zero: the control kernel in front of it clears it. The flag word
// accumulates over the call.
//
// No loop here has a bound that depends on data (16, 6, 3), no kernel waits for another workgroup, every index is checked
// against n before it is used.
#pragma once
#include "phd_kernels.h"

#define PHD_ASCENT_LINE_K 16          // include/phdhip.h: PHD_ASCENT_LINE
#define PHD_ASCENT_RATE 1e-2          // GradientAscentRate, Config.cs:94
#define PHD_ASCENT_CLIP 10.0          // GradientClip, Config.cs:95
#define PHD_ASCENT_GAIN 1e-3          // :964
#define PHD_ASCENT_EPS 1e-5           // :978

struct AscentBufs {
	int n;                        // estimates of this call
	const double* lin;            // [7] the linearisation pose ([problems][7] with `problem`)
	const int* problem;           // [n] the problem of estimate e (phd_ascent_multi.h); NULL: every estimate belongs to problem 0
	int* flags;                   // the batch's flag word
	unsigned long long* slab;     // ... and its slab counter (StepBufs::bigws_used of the evaluation launches)
	int* nactive;                 // estimates still active behind the last k_ascent_select
	double* pose6;                // [n][6] the accepted estimate
	double* loglike;              // [n] its value
	int*    iterations;           // [n]
	double* hess;                 // [n][6][6] raw finite-difference rows
	double* nextpose7;            // [n][7] the last TRIED pose (:933-934)
	double* prev;                 // [n]
	int*    active;               // [n]
	int*    chosen;               // [n] index of the line search's last candidate
	double* grad;                 // [n][6]
	double* gval;                 // [n] the gradient launch's value
	double* cand6;                // [n][16][6]
	double* cand7;                // [n][16][7]
	double* values;               // [n][16]
	double* hpose;                // [n][12][7]
	double* hgrad;                // [n][12][6]
	double* hval;                 // [n][12]
};

// the linearisation pose of estimate e
__device__ __forceinline__ const double* ascent_lin(const AscentBufs& s, int e) { return s.lin + 7 * (size_t) (s.problem ? s.problem[e] : 0); }

// Pose3D.Add (Pose3D.cs:282-291) as navigator.py::pose3d_add states it: x + q dx q*, q Exp(dr / 2) normalised
__device__ __forceinline__ void ascent_pose_add(const double* __restrict__ lin, const double d[6], double* __restrict__ out)
{
	PHD_REF_ARITH
	const Quat4 q{lin[3], lin[4], lin[5], lin[6]};
	const double l0 = 0.5 * d[3], l1 = 0.5 * d[4], l2 = 0.5 * d[5];
	const double phi = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
	Quat4 dq{1.0, 0.0, 0.0, 0.0};
	if (!(phi < 1e-12)) {   // Quaternion.Exp, Quaternion.cs:185-196
		const double s = sin(phi);
		dq = Quat4{cos(phi), s * (l0 / phi), s * (l1 / phi), s * (l2 / phi)};
	}
	const Quat4 nq = quat_mul(q, dq);
	const double nn = sqrt(nq.w * nq.w + nq.x * nq.x + nq.y * nq.y + nq.z * nq.z);
	const Quat4 dl = quat_mul(quat_mul(q, Quat4{0.0, d[0], d[1], d[2]}), Quat4{q.w, -q.x, -q.y, -q.z});
	out[0] = lin[0] + dl.x; out[1] = lin[1] + dl.y; out[2] = lin[2] + dl.z;
	out[3] = nq.w / nn; out[4] = nq.x / nn; out[5] = nq.y / nn; out[6] = nq.z / nn;
}

__global__ __launch_bounds__(256) void k_ascent_begin(const AscentBufs s)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i == 0) { *s.slab = 0; *s.nactive = 0; }
	if (i >= s.n) return;
	double d[6];
#pragma unroll
	for (int t = 0; t < 6; t++) d[t] = s.pose6[(size_t) i * 6 + t];
	ascent_pose_add(ascent_lin(s, i), d, s.nextpose7 + (size_t) i * 7);
	s.prev[i]       = -INFINITY;
	s.iterations[i] = 0;
	s.active[i]     = 1;
	s.chosen[i]     = -1;
}

// behind the first gradient launch: loglike is THAT launch's value (:928-929)
__global__ __launch_bounds__(256) void k_ascent_start(const AscentBufs s)
{
	PHD_REF_ARITH
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= s.n) return;
	const double ll = s.gval[i];
	s.loglike[i] = ll;
	s.active[i]  = (ll - s.prev[i] > PHD_ASCENT_GAIN) ? 1 : 0;   // (a NaN is inactive)
}

// one thread per (estimate, candidate): :936-942 and the step sizes of :943-951
__global__ __launch_bounds__(256) void k_ascent_candidates(const AscentBufs s)
{
	PHD_REF_ARITH
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t == 0) { *s.slab = 0; *s.nactive = 0; }   // the value launch behind this kernel; k_ascent_select counts anew
	const int e = t / PHD_ASCENT_LINE_K, c = t % PHD_ASCENT_LINE_K;
	if (e >= s.n || !s.active[e]) return;
	double g[6];
#pragma unroll
	for (int k = 0; k < 6; k++) g[k] = s.grad[(size_t) e * 6 + k];
	double sq = 0.0;
#pragma unroll
	for (int k = 0; k < 6; k++) sq = sq + g[k] * g[k];
	const double size = sqrt(sq);
	if (size > PHD_ASCENT_CLIP) {
		const double f = PHD_ASCENT_CLIP / size;
#pragma unroll
		for (int k = 0; k < 6; k++) g[k] = g[k] * f;
	}
	double m = PHD_ASCENT_RATE;
#pragma unroll
	for (int k = 0; k < PHD_ASCENT_LINE_K - 1; k++) {
		if (k < c) m = m / 2.0;
	}
	double d[6];
#pragma unroll
	for (int k = 0; k < 6; k++) {
		d[k] = s.pose6[(size_t) e * 6 + k] + m * g[k];
		s.cand6[(size_t) t * 6 + k] = d[k];
	}
	ascent_pose_add(ascent_lin(s, e), d, s.cand7 + (size_t) t * 7);
}

// one thread per estimate: c = 0; do { v = values[c]; c++; } while (v < loglike && c < 16); (:943-951) and what follows it
__global__ __launch_bounds__(256) void k_ascent_select(const AscentBufs s)
{
	PHD_REF_ARITH
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i == 0) *s.slab = 0;   // the gradient launch of the next iteration
	if (i >= s.n || !s.active[i]) return;
	const double ll = s.loglike[i];
	int    pick = PHD_ASCENT_LINE_K - 1;
	double v    = 0.0;
	bool   done = false;
#pragma unroll
	for (int c = 0; c < PHD_ASCENT_LINE_K; c++) {
		const double vc = s.values[(size_t) i * PHD_ASCENT_LINE_K + c];
		const bool last = !(vc < ll) || c == PHD_ASCENT_LINE_K - 1;
		if (!done && last) { pick = c; v = vc; done = true; }
	}
	const size_t cn = (size_t) i * PHD_ASCENT_LINE_K + pick;
#pragma unroll
	for (int k = 0; k < 7; k++) s.nextpose7[(size_t) i * 7 + k] = s.cand7[cn * 7 + k];
	double now = ll;
	if (v > ll) {
#pragma unroll
		for (int k = 0; k < 6; k++) s.pose6[(size_t) i * 6 + k] = s.cand6[cn * 6 + k];
		now = v;
		s.loglike[i] = v;
	}
	s.prev[i]   = ll;
	s.chosen[i] = pick;
	s.iterations[i] += 1;
	const int act = (now - ll > PHD_ASCENT_GAIN) ? 1 : 0;
	s.active[i] = act;
	if (act) atomicAdd(s.nactive, 1);
}

// the 12 poses Add(lin, pose6 +- eps e_i) of every estimate, row 2 i the plus and 2 i + 1 the minus one (:980-992)
__global__ __launch_bounds__(256) void k_ascent_hess_poses(const AscentBufs s)
{
	PHD_REF_ARITH
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t == 0) *s.slab = 0;
	const int e = t / 12, r = t % 12, i = r >> 1;
	if (e >= s.n) return;
	const double step = (r & 1) ? -1.0 * PHD_ASCENT_EPS : 1.0 * PHD_ASCENT_EPS;
	double d[6];
#pragma unroll
	for (int k = 0; k < 6; k++) {
		d[k] = s.pose6[(size_t) e * 6 + k];
		if (k == i) d[k] = d[k] + step;
	}
	ascent_pose_add(ascent_lin(s, e), d, s.hpose + (size_t) t * 7);
}

// H[i][j] = (g(+i)[j] - g(-i)[j]) / (2 eps), raw: the NaN test, the eigenvalue clip and the pseudo-inverse are the host's
__global__ __launch_bounds__(256) void k_ascent_hess_rows(const AscentBufs s)
{
	PHD_REF_ARITH
	const int t = blockIdx.x * 256 + threadIdx.x;
	const int e = t / 36, r = t % 36, i = r / 6, j = r % 6;
	if (e >= s.n) return;
	const double* g = s.hgrad + (size_t) e * 72;
	s.hess[t] = (g[(2 * i) * 6 + j] - g[(2 * i + 1) * 6 + j]) / (2 * PHD_ASCENT_EPS);
}

// The evaluations: alpha_assoc_body as k_quasi_setll_grad / k_quasi_setll call it. active != NULL: the workgroups of an
// estimate that has stopped return, all threads, before any barrier (`group` poses per estimate: 1 the gradient launch, 16 the
// candidates).
template <int ZB>
__global__ __launch_bounds__(256, PHD_QGRAD_WAVES) void k_ascent_setll_grad(const DevParams prm, const StepBufs a, int ncap, const int* active, int group)
{
	extern __shared__ __align__(16) double smem[];
	__shared__ __align__(16) double gws[QGRAD_LDS_DOUBLES];
	if (active && !active[blockIdx.x / group]) return;
	alpha_assoc_body<ZB, true, true>(prm, a, ncap, smem, gws);
}

template <int ZB>
__global__ __launch_bounds__(256, 4) void k_ascent_setll(const DevParams prm, const StepBufs a, int ncap, const int* active, int group)
{
	extern __shared__ __align__(16) double smem[];
	if (active && !active[blockIdx.x / group]) return;
	alpha_assoc_body<ZB, true>(prm, a, ncap, smem);
}
