// phd_maplog.h — the map log of a handle (phd_map_history_enable / _append, phd_map_history): what the reference keeps as
// Navigator.WayMaps (UpdateMapHistory, Navigator.cs:269-272: a copy of BestMapModel at the end of every SlamUpdate), kept on
// the device as the best particle's component records packed end to end plus one table row per appended entry.
//
//   rec  [components][10]   the records of all entries, entry k's at rec + entry[k].offset * 10 (offsets in whole records:
//                           every entry starts 16-byte aligned, as a bank's slots do)
//   entry[entries]          MapLogEntry: where entry k's records are, how many, which particle was best and its pose
//   bump [2]                records used so far. Two copies: every launch reads one and writes the other (the host counts the
//                           launches), so that a launch of several workgroups never reads what it writes.
//
// Everything an entry depends on is resolved here, on the device: the bank roles, BestParticle (info[0]), that particle's slot
// in the INMIX bank and its count. The host knows none of them behind a step it did not wait for.
// Every index read from device memory is clamped before it is used: a damaged word cannot read or write out of bounds.
#pragma once
#include "phd_history.h"

struct MapLogEntry {
	long long offset;    // first record of the entry in rec (count -1: where the log stood when the entry did not fit)
	int       count;     // records of the entry; -1: they did not fit the rest of the log and none was stored
	int       best;      // BestParticle when the entry was made
	double    pose[7];   // ... and its pose
};

// One entry. Every workgroup reads the header itself (sel -> info[0] -> inslot and count -> the bump word: no hand-over through
// memory), then copies its share of the records, 16 bytes per thread: thread t of the grid moves double2 number t of the map.
// The grid is sized for max_components; the workgroups beyond the map's end leave after the header (one workgroup looping over the
// map instead measured the same: profiles/map_history_cost.md).
// A template for its place in the code object alone: a plain kernel is emitted here, in front of every step kernel, and moved
// them all by 1 KB, which cost bench.py's config A 0.5 us a step with the log off; an instantiation is emitted behind them.
template <class Entry>
__global__ __launch_bounds__(256) void k_maplog_append(const StepBufs a, const int* __restrict__ info, int P, int Pcap, double* __restrict__ rec, long long components,
                                                       Entry* __restrict__ entry, const long long* __restrict__ bump_old, long long* __restrict__ bump_new)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	const Bank bi = bank_of(a, SEL_IN);
	const MixView vin = bank_view(a, SEL_IN);
	const int best = hist_clamp(info[0], P);
	const int slot = hist_clamp(a.inslot[best], Pcap);
	int n = vin.count[best];
	n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
	long long off = *bump_old;
	off = off < 0 ? 0 : (off > components ? components : off);
	const bool fits = n <= components - off;
	if (t == 0) {
		*bump_new = fits ? off + n : off;
		entry->offset = off;
		entry->count = fits ? n : -1;
		entry->best = best;
	}
	if (t < 7) entry->pose[t] = bi.poses[(size_t) best * 7 + t];
	if (!fits) return;
	const double2* from = (const double2*) (vin.rec + (size_t) slot * a.cap * MIX_REC);
	double2* to = (double2*) (rec + (size_t) off * MIX_REC);
	for (int i = t; i < n * (MIX_REC / 2); i += gridDim.x * 256) to[i] = from[i];
}
