// phd_ascent_multi.h — the pose searches of many frames in one call (phd_quasi_ascent_multi, phd_quasi_set_loglik_multi): the
// GuidedFitMixture of every frame of LoopyPHDNavigator.UpdateMessagesFromMap (LoopyPHDNavigator.cs:525-551) side by side. Each
// frame is a PROBLEM — its own map estimate, measurement set and linearisation pose — and every estimate (or pose of a batch)
// names the problem it belongs to. The estimates of different problems are as independent as those of one, so they share the
// launches of phd_ascent.h's chain: the control kernels take the linearisation pose of the estimate's problem (AscentBufs::problem),
// and the evaluation wrappers below hand alpha_assoc_body a StepBufs whose landmark set and measurement set are the problem's.
//
// What a wrapper derives from the problem table depends on blockIdx alone: the loads are uniform and what they give stays in
// scalar registers (the argument block is never indexed per lane, see bank_of in phd_kernels.h). No loop, no wait for another
// workgroup. The host has checked every offset and every problem index before anything was enqueued (phd_quasi_ascent_multi),
// so the pools are never indexed with an unchecked value.
#pragma once
#include "phd_ascent.h"

struct QuasiProblems {
	const int* problem;       // [n] problem of estimate e
	const int* lm_off;        // [nproblems + 1], in landmarks
	const int* z_off;         // [nproblems + 1], in measurements
	const double* lm;         // [sum J][3] the landmark pool
	const double* z;          // [sum M][3] the measurement pool
	const double* lin;        // [nproblems][7]
};

// `a` with the fields that differ between problems rebound to those of estimate e's problem
__device__ __forceinline__ StepBufs multi_rebind(const StepBufs& a, const QuasiProblems& pr, int e)
{
	const int q = __builtin_amdgcn_readfirstlane(pr.problem[e]);
	const int l0 = __builtin_amdgcn_readfirstlane(pr.lm_off[q]), l1 = __builtin_amdgcn_readfirstlane(pr.lm_off[q + 1]);
	const int z0 = __builtin_amdgcn_readfirstlane(pr.z_off[q]), z1 = __builtin_amdgcn_readfirstlane(pr.z_off[q + 1]);
	StepBufs b = a;
	b.qlm = pr.lm + 3 * (size_t) l0;
	b.qJ  = l1 - l0;
	b.z   = pr.z + 3 * (size_t) z0;
	b.M   = z1 - z0;
	return b;
}

// The evaluations: k_ascent_setll_grad / k_ascent_setll with the problem of the workgroup's estimate bound in. `group` poses per
// estimate: 1 a gradient launch or a batch, 16 the candidates, 12 the Hessian poses — it matters here even without `active`: e
// must be the ESTIMATE, the table has one entry for each. ZB is the block class of EVERY problem of the call.
template <int ZB>
__global__ __launch_bounds__(256, PHD_QGRAD_WAVES) void k_multi_setll_grad(const DevParams prm, const StepBufs a, int ncap, const QuasiProblems pr,
                                                                           const int* active, int group)
{
	extern __shared__ __align__(16) double smem[];
	__shared__ __align__(16) double gws[QGRAD_LDS_DOUBLES];
	const int e = blockIdx.x / group;
	if (active && !active[e]) return;
	const StepBufs b = multi_rebind(a, pr, e);
	alpha_assoc_body<ZB, true, true>(prm, b, ncap, smem, gws);
}

template <int ZB>
__global__ __launch_bounds__(256, 4) void k_multi_setll(const DevParams prm, const StepBufs a, int ncap, const QuasiProblems pr, const int* active, int group)
{
	extern __shared__ __align__(16) double smem[];
	const int e = blockIdx.x / group;
	if (active && !active[e]) return;
	const StepBufs b = multi_rebind(a, pr, e);
	alpha_assoc_body<ZB, true>(prm, b, ncap, smem);
}
