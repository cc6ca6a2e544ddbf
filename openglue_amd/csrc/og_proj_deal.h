// Work split of the weight-stationary q | k | v projection (proj_wstat.hip).  Plain C++ (host and device): no HIP type, so that a
// host-only program can include it (tests/test_proj_wstat_deal_cpu.py compiles one).
//
// A unit = one 32-token block x one 256-column slab.  A launch has up to two row ranges (the cross layer's launch: the rows of image 0
// take the q slab only): range A = token blocks [0, ba) x na slabs, range B = token blocks [ba, ba + bb) x nb slabs.  The G workgroups
// of a launch (one per CU) are numbered by SLOT; a range gets a run of slots, a run is cut into TEAMS of as many consecutive slots as
// the range has slabs, and a team shares one contiguous run of token blocks -- member j of the team produces slab j of it.  The blocks
// of a range are dealt to its teams in equal contiguous runs (they differ by at most one block).
// slot <-> workgroup id: slot = (id & 7) * (G / 8) + (id >> 3).  Workgroups are dealt to the 8 XCDs round-robin by id, so consecutive
// slots -- the members of a team -- sit on ONE XCD (except the few teams that straddle a multiple of G / 8) and start together: the x
// rows of a token run are read from memory once and from that XCD's L2 by the other members.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OG_DEAL_HD __host__ __device__
#else
#define OG_DEAL_HD
#endif

struct OgProjDeal {
    int ba, na, bb, nb;       // token blocks and slabs of the two ranges (a range with 0 blocks or 0 slabs is empty)
    int b_first;              // first token block of range B (the blocks below it belong to range A, even when A has no slab)
    int ta, tb;               // teams of the two ranges: ta * na + tb * nb <= G, ta <= ba, tb <= bb
};

// The team counts that minimise the longest run of token blocks one workgroup walks.  G: workgroups of the launch.
inline OgProjDeal og_proj_deal(int ba, int na, int bb, int nb, int G) {
    OgProjDeal d{ba, na, bb, nb, ba > 0 ? ba : 0, 0, 0};
    if (ba <= 0 || na <= 0) { d.ba = 0; d.na = 0; }
    if (bb <= 0 || nb <= 0) { d.bb = 0; d.nb = 0; }
    auto cap = [](int teams, int blocks) { return teams < blocks ? teams : blocks; };
    if (!d.ba && !d.bb) return d;
    if (!d.ba) { d.tb = cap(G / d.nb, d.bb); return d; }
    if (!d.bb) { d.ta = cap(G / d.na, d.ba); return d; }
    int best = 0x7fffffff;
    for (int ta = 1; ta * d.na < G && ta <= d.ba; ++ta) {
        const int tb = cap((G - ta * d.na) / d.nb, d.bb);
        if (tb < 1) break;
        const int ra = (d.ba + ta - 1) / ta, rb = (d.bb + tb - 1) / tb;
        const int longest = ra > rb ? ra : rb;
        if (longest < best) { best = longest; d.ta = ta; d.tb = tb; }
    }
    return d;
}

// ... of a launch over M token rows: the rows below split_row form range A (split_row a multiple of 32; <= 0: no range A, >= M: no range B)
inline OgProjDeal og_proj_deal_rows(int M, int split_row, int na, int nb, int G) {
    const int blocks = (M + 31) / 32;
    const int ba = split_row <= 0 ? 0 : split_row >= M ? blocks : split_row / 32;
    return og_proj_deal(ba, na, blocks - ba, nb, G);
}

OG_DEAL_HD inline int og_proj_deal_slot(int id, int G) { return (id & 7) * (G / 8) + (id >> 3); }

// The work of one slot: slab index `slab` inside its range's slab list, token blocks [blk0, blk1) (numbered over the whole launch),
// range 0 = A / 1 = B.  false: the slot has nothing to do.
OG_DEAL_HD inline bool og_proj_deal_unit(const OgProjDeal& d, int slot, int& range, int& slab, int& blk0, int& blk1) {
    const int sa = d.ta * d.na;
    int s = slot, teams, ns, blocks, first;
    if (s < sa) { range = 0; teams = d.ta; ns = d.na; blocks = d.ba; first = 0; }
    else { s -= sa; range = 1; teams = d.tb; ns = d.nb; blocks = d.bb; first = d.b_first; }
    if (ns <= 0 || s >= teams * ns) return false;
    const int team = s / ns;
    slab = s - team * ns;
    blk0 = first + (int)((long long)team * blocks / teams);
    blk1 = first + (int)((long long)(team + 1) * blocks / teams);
    return blk1 > blk0;
}
