// The steps of the grid's table build, one copy each: the single build (pcr_grid.hip) and the fused batch (pcr_batch.hip) call them,
// so a batch's tables are the per-pair path's by construction.  A kernel keeps only how it finds its element (its record, the
// record's position `li` inside its cloud of `n` points, and the cloud's tables as a pcr_grid_view).
#pragma once
#include "pcr_grid_dev.h"

constexpr unsigned long long MORTON_BIAS3 = 7ull << 60;   // spread21(PCR_COORD_BIAS) on x, y and z: the key bits no cloud varies

// ---------------------------------------------------------------- capacities (host and device)
__host__ __device__ static inline unsigned int next_pow2(unsigned long long v) {
    return v <= 1 ? 1u : (unsigned int)(1ull << (64 - __builtin_clzll(v - 1)));
}
// Slots of a level's cell table (buckets of 4 slots, load factor <= 0.25) and of its 2x2x2-block table (blocks <= cells: load
// factor <= 0.5, usually ~0.15) from the level's cell count; neither smaller than `min_cap`.
struct pcr_table_caps {
    unsigned int cap, bcap;
};
__host__ __device__ static inline pcr_table_caps pcr_table_caps_of(unsigned long long cells, unsigned int min_cap) {
    pcr_table_caps c = {next_pow2(cells * 4 + 4), next_pow2(cells * 2 + 4)};
    if (c.cap < min_cap) c.cap = min_cap;
    if (c.bcap < min_cap) c.bcap = min_cap;
    return c;
}

// ---------------------------------------------------------------- keys and run starts
// 63-bit Morton key of a point's level-0 cell on the curve with origin `lo` and 1 / cell `inv` (the caller masks the bits it sorts)
__device__ static inline unsigned long long morton_key(double x, double y, double z, double lox, double loy, double loz, double inv) {
    bool clamped = false;
    const unsigned long long cx = (unsigned long long)cell_coord(x, lox, inv, &clamped);
    const unsigned long long cy = (unsigned long long)cell_coord(y, loy, inv, &clamped);
    const unsigned long long cz = (unsigned long long)cell_coord(z, loz, inv, &clamped);
    return spread21(cx) | (spread21(cy) << 1) | (spread21(cz) << 2);
}

// Cells of every level = run starts of key >> 6l: the wave votes, its first lane adds the votes to the caller's counter of the level
// (`kp`: the key of the record before, unused at li == 0; every lane of the wave must call this)
__device__ static inline void count_run_starts(unsigned long long k, unsigned long long kp, unsigned long long li, bool valid, int levels,
                                               unsigned int* cnt) {
    for (int l = 0; l < levels; ++l) {
        const bool start = valid && (li == 0 || (k >> (6 * l)) != (kp >> (6 * l)));
        const unsigned long long b = __ballot(start);
        if (b && (threadIdx.x & 63) == 0) atomicAdd(&cnt[l], (unsigned int)__popcll(b));
    }
}

// ---------------------------------------------------------------- tables
// grid-stride clear (thread t0 of `stride`) of the first n_cells / n_blocks slots of the pools: cell slots all-ones, block slots
// {free key, start = ~0, flags = 0, cnt[8] = 0}
__device__ static inline void clear_pools(pcr_cell_slot* cell_pool, unsigned long long n_cells, pcr_block_slot* block_pool, unsigned long long n_blocks,
                                          unsigned long long t0, unsigned long long stride) {
    typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
    u2* cp = reinterpret_cast<u2*>(cell_pool);
    for (unsigned long long i = t0; i < n_cells; i += stride) cp[i] = u2{~0ull, ~0ull};
    u2* bp = reinterpret_cast<u2*>(block_pool);
    for (unsigned long long i = t0; i < 2 * n_blocks; i += stride) bp[i] = (i & 1) ? u2{0ull, 0ull} : u2{PCR_EMPTY_KEY, 0x00000000ffffffffull};
}

// buckets of 4 slots, filled from slot 0; mask = number of buckets - 1
__device__ static inline unsigned int slot_find_or_insert(pcr_cell_slot* tab, unsigned int mask, unsigned long long key, unsigned int h) {
    unsigned int b = h & mask;
    for (unsigned int probe = 0; probe <= mask; ++probe) {
        for (unsigned int k = 0; k < 4; ++k) {
            const unsigned int slot = b * 4 + k;
            unsigned long long old = atomicCAS(&tab[slot].key, PCR_EMPTY_KEY, key);
            if (old == PCR_EMPTY_KEY || old == key) return slot;
        }
        b = (b + 1) & mask;
    }
    return 0xffffffffu;  // table full: cannot happen at load factor <= 0.25
}

// Record li of n, with full key k between kp and kn (unused at the ends): on every level where it is the first or the last record
// of its cell's run it writes that end of the run into the cell's slot.
__device__ static inline void insert_cell_runs(const pcr_grid_view& gv, unsigned long long k, unsigned long long kp, unsigned long long kn,
                                               unsigned long long li, unsigned long long n) {
    const int levels = gv.levels;
    for (int l = 0; l < levels; ++l) {
        const unsigned long long ck = k >> (6 * l);
        const bool start = (li == 0) || (ck != (kp >> (6 * l)));
        const bool end = (li + 1 == n) || (ck != (kn >> (6 * l)));
        if (start || end) {
            const unsigned int X = compact21(ck), Y = compact21(ck >> 1), Z = compact21(ck >> 2);
            pcr_cell_slot* tab = const_cast<pcr_cell_slot*>(gv.table[l]);
            const unsigned int h = slot_find_or_insert(tab, gv.mask[l], cell_pack(X, Y, Z), cell_hash(X, Y, Z));
            if (h != 0xffffffffu) {
                if (start) tab[h].start = (unsigned int)li;
                if (end) tab[h].end = (unsigned int)(li + 1);
            }
        }
    }
}

// The thread at the first record of a cell's run looks the (now complete) slot up and registers the cell in its 2x2x2 block: work
// proportional to the cells, coalesced key reads.  (Walking every slot of every table instead -- four fifths of them empty -- took
// 18.5 us at 120 000 points; in the batch, with a binary search per block of 256 slots for the slot's table, 0.62 of the 5.1 ms of
// 256 pairs.)  A child of 65 535 points or more sets the block's flag: the search then reads the cell table for that block.
__device__ static inline void register_cell_in_block(const pcr_grid_view& gv, unsigned long long k, unsigned long long kp, unsigned long long li) {
    const int levels = gv.levels;
    for (int l = 0; l < levels; ++l) {
        const unsigned long long ck = k >> (6 * l);
        if (li != 0 && ck == (kp >> (6 * l))) break;   // not a run start here: not one on any coarser level either
        const unsigned int X = compact21(ck), Y = compact21(ck >> 1), Z = compact21(ck >> 2);
        unsigned int cs = 0, ce = 0;
        if (!lookup_cell(gv.table[l], gv.mask[l], X, Y, Z, &cs, &ce)) continue;
        pcr_block_slot* bt = const_cast<pcr_block_slot*>(gv.btable[l]);
        const unsigned int bmask = gv.bmask[l];
        const unsigned int BX = X >> 1, BY = Y >> 1, BZ = Z >> 1;
        const int child = (int)((X & 1) | ((Y & 1) << 1) | ((Z & 1) << 2));
        const unsigned long long bk = cell_pack(BX, BY, BZ);
        unsigned int b = cell_hash(BX, BY, BZ) & bmask;
        for (unsigned int probe = 0; probe <= bmask; ++probe) {
            const unsigned long long old = atomicCAS(&bt[b].key, PCR_EMPTY_KEY, bk);
            if (old == PCR_EMPTY_KEY || old == bk) break;
            b = (b + 1) & bmask;
        }
        const unsigned int cnt = ce - cs;
        if (cnt >= 0xffffu) atomicOr(&bt[b].flags, 1u);
        bt[b].cnt[child] = (unsigned short)(cnt >= 0xffffu ? 0xffffu : cnt);
        atomicMin(&bt[b].start, cs);
    }
}
