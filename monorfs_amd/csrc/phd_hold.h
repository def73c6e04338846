// phd_hold.h — one particle sits a mapping step out (phd_step_hold_async): its mixture is copied out of the current state in
// front of the step and copied back into the current state behind it. No step kernel knows of it.
//
//   rec  [max_components][10]   the held slot's component records as they stood in front of the step
//   count[1]                    how many of them
//
// Both kernels resolve where the current state lives here, on the device: the bank whose small arrays are current (IN), the bank
// that holds the mixtures (INMIX) and the particle's slot in it (inslot). The roles rotate inside k_normalise_resample and the
// host knows none of them between posted steps. k_hold_save is launched with the roles in front of the step, k_hold_restore with
// those behind it: behind a mapping step that ran, the held slot's mixture is the one the step wrote (INMIX = IN, slots the
// identity) and is overwritten; behind a step that dropped itself the roles stayed, and the records go back where they came from.
// The count and the slot are clamped before they are used: a damaged word cannot read or write out of bounds.
#pragma once
#include "phd_kernels.h"

// One workgroup. (Templates for their place in the code object alone, as k_maplog_append: an instantiation is emitted behind
// the step kernels and does not move them.)
template <class Count>
__global__ __launch_bounds__(256) void k_hold_save(const StepBufs a, int held, int Pcap, double* __restrict__ rec, Count* __restrict__ count)
{
	const int tid = threadIdx.x;
	const MixView vin = bank_view(a, SEL_IN);
	int n = vin.count[held];
	n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
	int slot = a.inslot[held];
	slot = slot < 0 ? 0 : (slot >= Pcap ? Pcap - 1 : slot);
	copy_comps(rec, vin.rec + (size_t) slot * a.cap * MIX_REC, n, tid, 256);
	if (tid == 0) *count = n;
}

template <class Count>
__global__ __launch_bounds__(256) void k_hold_restore(const StepBufs a, int held, int Pcap, const double* __restrict__ rec, const Count* __restrict__ count)
{
	const int tid = threadIdx.x;
	const MixView vin = bank_view(a, SEL_IN);
	int n = *count;
	n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
	int slot = a.inslot[held];
	slot = slot < 0 ? 0 : (slot >= Pcap ? Pcap - 1 : slot);
	copy_comps(vin.rec + (size_t) slot * a.cap * MIX_REC, rec, n, tid, 256);
	if (tid == 0) vin.count[held] = n;
}
