// prune_lds(c) for c = 1 .. 6000, one line each: bytes, NS, x, rad2, scan. Host only; built against two trees in turn, the two
// tables are compared with cmp (profiles/prune_parts.md):
//   hipcc --offload-arch=gfx950 -std=c++17 -I <tree>/monorfs_amd/csrc [-DPRUNE_CARVE] scripts/probes/prune_lds_table.hip -o table && ./table > table.txt
// With -DPRUNE_CARVE (a tree whose PruneLds names every array) it also asserts, for every c, what the body relies on: the ranked
// ordering's arrays fit the pool, kw | ks stay inside the sort arrays' place, and no array of a group passes the tail.
#include <cassert>
#include <cstdio>
#define PHD_ONLY_EP   // (the emit and prune kernels alone: phd_prune.h needs the headers in front of it)
#include "phd_kernels.h"

int main()
{
	for (int c = 1; c <= 6000; c++) {
		const PruneLds l = prune_lds(c);
		printf("%d %d %d %d %d %d\n", c, l.bytes, l.NS, l.x, l.rad2, l.scan);
#ifdef PRUNE_CARVE
		const int tail = 2 * l.scan;
		assert(l.capN == (l.NS * 2) / 3 && l.cc >= c && l.cc % 2 == 0);
		assert(l.sw == 2 * l.x && l.w2 == l.sw + l.NS && l.w2 + l.NS <= tail);
		assert(l.kw == l.sw && l.kw % 2 == 0 && l.ks == l.kw + 2 * l.capN && l.ks + l.capN <= l.hist);
		assert(l.hist == l.w2 + l.NS && l.out == l.hist + PruneLds::HIST && l.ki == l.out + l.capN && l.ki + l.capN <= l.ranked_end && l.ranked_end <= tail);
		assert(l.nbr % 2 == 0 && l.cand == l.nbr + 4 * l.cc && l.cand % 4 == 0 && l.owner == l.cand + 4 * l.cc && l.cw == l.owner + l.cc);
		assert(l.absb == l.cw + PruneLds::CW && l.absb % 2 == 0 && l.ord == l.absb + PruneLds::ABSB && l.rowpos == l.ord + l.cc / 2);
		assert(l.rowpos + l.cc / 2 <= l.merge_end && l.merge_end <= tail);
		assert(l.bytes == (tail + PruneLds::SCAN + PruneLds::TAIL_PAD) * 4 && l.rad2 == 0 && 2 * l.x >= l.cc);
#endif
	}
	return 0;
}
