// phd_maperror.h — the map-error metric of the reference's post-analysis over the map log (phd_map_error): for every logged
// map Map.BestMapEstimate (Map.cs:119-142), the alignment of Plot.MapError (postanalysis/Plot.cs:478-529) and Plot.OSPA
// (:531-581) against one truth set, one workgroup per log entry, everything in FP64. monorfs_amd/host/Ospa.hpp is the same
// metric on the host and states the formulas.
//
// LDS of a workgroup (62 KB, static):
//   est  [MAX][3]   the estimate, in the order of the reference's sorted list, moved by the alignment in place
//   tru  [MAX][3]   the truth set
//   u    [MAX]      row potentials of the assignment; behind it the cost of every row's pair, for the final sum
//   way, prow [MAX] int16: the column a column was reached from | the row a column is matched to (-1: none)
//   red  [256]      block_tree_sum's scratch, then the waves' minima of the column scans (two sets of four)
// The columns of the assignment live in registers: thread t owns columns t, t + 256, t + 512, t + 768 (the point, the column
// potential, the reduced cost so far and whether the column is in the tree).
//
// Every loop is bounded by a number known when the workgroup starts (the entry's count, J, m, n); a workgroup that would go
// beyond one stores PHD_MAPERR_FLAG_BOUND into the flag word and leaves. Every index read from device memory is clamped.
// No atomics, no waiting on another workgroup.
#pragma once
#include "phd_maplog.h"

#define PHD_MAPERR_MAX 1024          // points of either set (include/phdhip.h: PHD_MAP_ERROR_MAX)
#define PHD_MAPERR_COLS (PHD_MAPERR_MAX / 256)
#define PHD_MAPERR_FLAG_BOUND 1      // a loop met its bound (non-finite records in the log are the one way there)

// what the host hands over per entry: has (0 / 1), then R[9], c[3], t[3] of p' = R (p - c) + c - t
#define PHD_MAPERR_ALIGN 16

// x^P and x^(1/P); P = 1 and P = 2 are what a correctly rounded pow gives, without the call
__device__ __forceinline__ double maperr_pow(double x, double P) { return P == 1.0 ? x : (P == 2.0 ? x * x : pow(x, P)); }
__device__ __forceinline__ double maperr_root(double x, double P) { return P == 1.0 ? x : (P == 2.0 ? sqrt(x) : pow(x, 1.0 / P)); }

// the cost of a pair: min(C, d)^P, or C^P where the gain C^P - that is not above 1e-5 (Plot.cs:561: such entries are not stored)
__device__ __forceinline__ double maperr_cost(double ax, double ay, double az, double bx, double by, double bz, double C, double P, double CP)
{
	const double d0 = ax - bx, d1 = ay - by, d2 = az - bz;
	const double dist = maperr_pow(fmin(C, sqrt(d0 * d0 + d1 * d1 + d2 * d2)), P);
	return (CP - dist > 1e-5) ? dist : CP;
}

// A template for its place in the code object alone, as k_maplog_append is (phd_maplog.h).
template <class Entry>
__global__ __launch_bounds__(256) void k_map_error(const double* __restrict__ rec, long long components, int cap, const Entry* __restrict__ entry,
                                                   const double* __restrict__ truth, int ntruth, double C, double P, const double* __restrict__ align,
                                                   double* __restrict__ out_ospa, double* __restrict__ out_card, double* __restrict__ out_spatial,
                                                   int* __restrict__ out_size, int* __restrict__ flag)
{
	constexpr int MAX = PHD_MAPERR_MAX, NC = PHD_MAPERR_COLS;
	__shared__ __align__(16) double est[MAX * 3];
	__shared__ __align__(16) double tru[MAX * 3];
	__shared__ double u[MAX];
	__shared__ double red[256];
	__shared__ short way[MAX], prow[MAX];
	__shared__ double s_sum;
	__shared__ int s_bad;

	const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const double nan = __longlong_as_double(0x7ff8000000000000ll);
	auto leave = [&](double o, double c, double s, int size) {
		if (tid == 0) { out_ospa[k] = o; out_card[k] = c; out_spatial[k] = s; out_size[k] = size; }
	};

	// ---- the entry's records
	int count = entry[k].count;
	if (count < 0) { leave(nan, nan, nan, -1); return; }
	count = count > cap ? cap : count;
	if ((long long) count > components) count = (int) components;
	long long off = entry[k].offset;
	off = off < 0 ? 0 : (off > components - count ? components - count : off);
	const double* r = rec + (size_t) off * MIX_REC;

	// ---- Map.BestMapEstimate: J = (int) ExpectedSize. The reference adds the weights one by one; the tree sum differs from that
	// by a few ulp, which changes the integer part only next to an integer: there the weights are re-added in map order
	// (alpha_assoc_body's rule, phd_alpha.h phase 1).
	if (tid == 0) s_bad = 0;
	double wpart = 0;
	for (int c = tid; c < count; c += 256) wpart += r[(size_t) c * MIX_REC];
	double e = block_tree_sum(red, wpart, tid);
	if (fabs(e - rint(e)) <= 1e-9 * fmax(1.0, fabs(e))) {
		if (tid == 0) {
			double q = 0;
			for (int c = 0; c < count; c++) q += r[(size_t) c * MIX_REC];
			s_sum = q;
		}
		__syncthreads();
		e = s_sum;
	}
	// (a sum that is no number, or beyond every size the kernel holds: the entry is over the bound, with the largest size as its own)
	const int J = !(e >= 1.0) ? 0 : (e >= 2147483647.0 ? 2147483647 : (int) e);
	if (J > MAX) { leave(nan, nan, nan, J); return; }

	// The estimate is the first J entries of the list the reference ends with: every component's weight w, and w - 1, w - 2, ...
	// (a pick re-enters with its weight less one), stably sorted by falling weight. A re-entered copy stands behind everything
	// that was in the list before it, so equal weights are ordered by the number of subtractions, then by map index. An entry's
	// place is the number of entries before it: counted here for every entry until one of a component's chain falls behind J.
	// (w - k is exact while it is not negative, so comparing the chains' members needs no tolerance.)
	for (int t = tid; t < J * 3; t += 256) est[t] = 0.0;
	for (int t = tid; t < ntruth * 3; t += 256) tru[t] = truth[t];
	__syncthreads();
	for (int c = tid; c < count; c += 256) {
		const double wc = r[(size_t) c * MIX_REC];
		for (int kk = 0; kk <= J; kk++) {
			const double x = wc - (double) kk;
			int rank = 0;
			for (int o = 0; o < count; o++) {
				const double wo = r[(size_t) o * MIX_REC];
				const double d = wo - x;
				if (!(d >= 0.0)) continue;
				// g: the last member of o's chain that is not below x (floor(d), put right where the subtraction rounded)
				int g = (int) fmin(floor(d), (double) (J + 1));
				if (wo - (double) (g + 1) >= x) g++;
				else if (!(wo - (double) g >= x)) g--;
				const bool eq = g >= 0 && wo - (double) g == x;
				rank += g + 1 - (eq && !(g < kk || (g == kk && o < c)) ? 1 : 0);
			}
			if (rank >= J) break;
			est[rank * 3 + 0] = r[(size_t) c * MIX_REC + 1];
			est[rank * 3 + 1] = r[(size_t) c * MIX_REC + 2];
			est[rank * 3 + 2] = r[(size_t) c * MIX_REC + 3];
		}
	}
	__syncthreads();

	// ---- the alignment of Plot.MapError (:505-515): p' = R (p - c) + c - t
	const double* al = align + (size_t) k * PHD_MAPERR_ALIGN;
	if (al[0] != 0.0) {
		for (int j = tid; j < J; j += 256) {
			const double d0 = est[j * 3] - al[10], d1 = est[j * 3 + 1] - al[11], d2 = est[j * 3 + 2] - al[12];
#pragma unroll
			for (int i = 0; i < 3; i++) est[j * 3 + i] = (al[1 + i * 3] * d0 + al[2 + i * 3] * d1 + al[3 + i * 3] * d2) + al[10 + i] + (-1.0) * al[13 + i];
		}
		__syncthreads();
	}

	// ---- Plot.OSPA: the rows are the smaller set (the truth set when both are as large), the columns the larger one
	const bool rows_are_est = ntruth > J;
	const double* S = rows_are_est ? est : tru;
	const double* L = rows_are_est ? tru : est;
	const int m = rows_are_est ? J : ntruth, n = rows_are_est ? ntruth : J;
	if (m == 0) {
		const double c = (n == 0) ? 0.0 : C;   // :539-542
		leave(c, c, maperr_root(maperr_pow(c, P) - maperr_pow(c, P), P), J);
		return;
	}
	const double CP = maperr_pow(C, P);
	const double INF = __longlong_as_double(0x7ff0000000000000ll);

	// Shortest augmenting paths with row and column potentials (the scheme of Ospa.hpp::AssignmentMinCost) for the m rows
	// alone: the n - m rows that pad the problem to a square cost C^P in every column and take whatever columns are left.
	double lx[NC], ly[NC], lz[NC], v[NC], minv[NC];
	bool used[NC];
#pragma unroll
	for (int q = 0; q < NC; q++) {
		const int j = tid + 256 * q;
		lx[q] = j < n ? L[j * 3] : 0.0; ly[q] = j < n ? L[j * 3 + 1] : 0.0; lz[q] = j < n ? L[j * 3 + 2] : 0.0;
		v[q] = 0.0;
		prow[j] = -1; way[j] = -1; u[j] = 0.0;
	}
	__syncthreads();
	double* wmin = red;                  // [2][4] the waves' minima, by the parity of the scan
	int* wcol = (int*) (red + 8);        // [2][4] ... and their columns
	int scans = 0;
	for (int i = 0; i < m; i++) {
#pragma unroll
		for (int q = 0; q < NC; q++) { minv[q] = INF; used[q] = false; }
		int j0 = -1;                     // the column the tree was last grown by (-1: the root, row i itself)
		bool found = false;
		for (int it = 0; it <= i; it++) {   // (a scan adds a matched column to the tree or ends the search: i matched columns)
			const int i0 = j0 < 0 ? i : prow[j0];
			const double sx = S[i0 * 3], sy = S[i0 * 3 + 1], sz = S[i0 * 3 + 2], ui = u[i0];
			double best = INF;
			int bestj = MAX;
#pragma unroll
			for (int q = 0; q < NC; q++) {
				const int j = tid + 256 * q;
				if (j == j0) used[q] = true;
				if (j < n && !used[q]) {
					const double cur = maperr_cost(sx, sy, sz, lx[q], ly[q], lz[q], C, P, CP) - ui - v[q];
					if (cur < minv[q]) { minv[q] = cur; way[j] = (short) j0; }
					if (minv[q] < best) { best = minv[q]; bestj = j; }   // (columns rise with q: the first of equal minima stays)
				}
			}
#pragma unroll
			for (int s = 32; s > 0; s >>= 1) {
				const double ob = __shfl_xor(best, s, 64);
				const int oj = __shfl_xor(bestj, s, 64);
				if (ob < best || (ob == best && oj < bestj)) { best = ob; bestj = oj; }
			}
			const int set = (scans++ & 1) * 4;
			if (lane == 0) { wmin[set + wv] = best; wcol[set + wv] = bestj; }
			__syncthreads();
			double delta = wmin[set];
			int j1 = wcol[set];
#pragma unroll
			for (int w = 1; w < 4; w++) {
				const double ob = wmin[set + w];
				const int oj = wcol[set + w];
				if (ob < delta || (ob == delta && oj < j1)) { delta = ob; j1 = oj; }
			}
			if (j1 >= n || !(delta < INF)) break;   // (no column left to reach: costs that are no numbers)
#pragma unroll
			for (int q = 0; q < NC; q++) {
				const int j = tid + 256 * q;
				if (j < n) {
					if (used[q]) { u[prow[j]] += delta; v[q] -= delta; }
					else minv[q] -= delta;
				}
			}
			if (tid == 0) u[i] += delta;
			j0 = j1;
			if (prow[j1] < 0) { found = true; break; }
		}
		if (!found) {
			if (tid == 0) *flag = PHD_MAPERR_FLAG_BOUND;
			leave(nan, nan, nan, J);
			return;
		}
		__syncthreads();                 // (every thread has read prow[j0]; the scans' writes of `way` are in LDS)
		if (tid == 0) {
			int j = j0;
			for (int step = 0; step <= i && j >= 0; step++) {   // back along the path: at most the i matched columns and the free one
				const int jp = way[j];
				prow[j] = jp < 0 ? (short) i : prow[jp];
				j = jp;
			}
			if (j >= 0) s_bad = 1;
		}
		__syncthreads();
	}
	if (s_bad) {
		if (tid == 0) *flag = PHD_MAPERR_FLAG_BOUND;
		leave(nan, nan, nan, J);
		return;
	}

	// ---- the value: the assigned pairs' costs added in row order, C^P for every column without a row
	double* pair = u;
#pragma unroll
	for (int q = 0; q < NC; q++) {
		const int j = tid + 256 * q;
		if (j < n && prow[j] >= 0) {
			const int i = prow[j];
			pair[i] = maperr_cost(S[i * 3], S[i * 3 + 1], S[i * 3 + 2], lx[q], ly[q], lz[q], C, P, CP);
		}
	}
	__syncthreads();
	if (tid == 0) {
		double total = 0;
		for (int i = 0; i < m; i++) total += pair[i];
		total += (double) (n - m) * CP;
		const double ospa = maperr_root(total / n, P);
		const double card = C * maperr_root((double) (n - m) / n, P);
		out_ospa[k] = ospa;
		out_card[k] = card;
		out_spatial[k] = maperr_root(maperr_pow(ospa, P) - maperr_pow(card, P), P);   // :519
		out_size[k] = J;
	}
}
