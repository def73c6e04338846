// phd_history.h — the trajectory log of a handle (phd_history_enable / _append, phd_trajectories): what the reference keeps
// as Vehicle.WayPoints per particle (Vehicle.cs:335, TrackVehicle.cs:101) and deep-copies on every resampling
// (PHDNavigator.cs:740), kept on the device as one row of poses per appended entry plus the ancestry between rows.
//
//   pose  [capacity][Ps][7]   the particle poses at every append (Ps = max_particles: the row stride)
//   parent[capacity][Ps]      slot, in entry k - 1, of the particle that sits in slot i at entry k
//   dirty [capacity]          0: parent[k] is the identity (no step resampled between entries k - 1 and k) and is never read
//   pend  [2][Ps] + dirty[2]  the composition of the resamplings since the last append: the particle now in slot i sat in slot
//                             pend[i] at the newest entry. Two copies: every launch reads one and writes the other (the host
//                             counts the launches), so that a launch of several workgroups never reads what it writes.
//
// A path is read backwards: only the entries whose dirty word is set cost a dependent trip to memory (k_hist_trace).
// Every slot read from the log is clamped into [0, P) before it is used as an index: a damaged log cannot read out of bounds.
#pragma once
#include "phd_kernels.h"

__device__ __forceinline__ int hist_clamp(int a, int P) { return a < 0 ? 0 : (a >= P ? P - 1 : a); }

// pend <- the clean identity (phd_history_enable, and the restart of phd_reset / phd_upload_state_soa)
__global__ __launch_bounds__(256) void k_hist_identity(int* pend, int* pdirty, int n)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i == 0) *pdirty = 0;
	if (i < n) pend[i] = i;
}

// Behind the end of a step (k_normalise_resample or the k_nr_* launches, same stream): new[i] = old[src[i]] if the step resampled;
// a step that did not, and a dropped one (a raised flag: it wrote neither src nor info), copy through. src is not read then.
__global__ __launch_bounds__(256) void k_hist_compose(const int* flags, const int* info, const int* src, const int* pend_old, const int* pdirty_old,
                                                      int* pend_new, int* pdirty_new, int P)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	const int dropped = *flags, d = *pdirty_old;
	const int resampled = dropped ? 0 : info[1];
	if (i == 0) *pdirty_new = (resampled || d) ? 1 : 0;
	if (i >= P) return;
	int v;
	if (resampled) {
		const int s = hist_clamp(src[i], P);
		v = d ? pend_old[s] : s;
	}
	else v = pend_old[i];
	pend_new[i] = v;
}

// One entry: the poses of the current state (the IN bank, resolved here as in k_motion: correct right behind an asynchronous
// step), its ancestry from pend, and pend left as the clean identity. One thread per double of the row.
__global__ __launch_bounds__(256) void k_hist_append(const StepBufs a, int P, double* pose_row, int* parent_row, int* dirty_k,
                                                     const int* pend_old, const int* pdirty_old, int* pend_new, int* pdirty_new)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	const double* poses = bank_of(a, SEL_IN).poses;
	const int d = *pdirty_old;
	if (i == 0) { *dirty_k = d; *pdirty_new = 0; }
	if (i < P * 7) pose_row[i] = poses[i];
	if (i < P) {
		parent_row[i] = d ? pend_old[i] : i;
		pend_new[i] = i;
	}
}

// The paths of nq particles of the current state, oldest entry first: out_pose[nq][L][7], out_slot[nq][L]. One wave per
// particle; the entries newest to oldest in chunks of 64, lane l on entry hi - l. The ancestor slot `a` is one value per wave
// and is chased (a = parent[k][a]) only at the entries a ballot of the dirty words names: the dependent trips to memory are as
// many as the resampled entries, not as the path is long. Every lane then copies its own entry.
// pend == NULL (phd_trajectories_at): the query names slots of entry L - 1 itself, no pending map lies before the first trip.
__global__ __launch_bounds__(256) void k_hist_trace(const double* __restrict__ pose, const int* __restrict__ parent, const int* __restrict__ dirty,
                                                    const int* __restrict__ pend, const int* __restrict__ pdirty, const int* __restrict__ query,
                                                    int nq, int L, int P, int Ps, double* __restrict__ out_pose, int* __restrict__ out_slot)
{
	const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (q >= nq) return;   // (a whole wave)
	const int p = hist_clamp(query[q], P);
	int a = __builtin_amdgcn_readfirstlane(hist_clamp((pend && *pdirty) ? pend[p] : p, P));
	for (int hi = L - 1; hi >= 0; hi -= 64) {
		const int k = hi - lane;
		// (entry 0 has no entry before it: whatever resampled before the first append composes nothing)
		unsigned long long m = ballot64(k >= 1 && dirty[k] != 0);
		int mine = a;
		while (m) {
			const int j = __ffsll((long long) m) - 1;   // the newest of the chunk's resampled entries not yet passed
			m &= m - 1;
			a = __builtin_amdgcn_readfirstlane(hist_clamp(parent[(size_t) (hi - j) * Ps + a], P));
			if (lane > j) mine = a;
		}
		if (k >= 0) {
			const double* from = pose + ((size_t) k * Ps + mine) * 7;
			double* to = out_pose + ((size_t) q * L + k) * 7;
			double v[7];
#pragma unroll
			for (int t = 0; t < 7; t++) v[t] = from[t];
#pragma unroll
			for (int t = 0; t < 7; t++) to[t] = v[t];
			out_slot[(size_t) q * L + k] = mine;
		}
	}
}
