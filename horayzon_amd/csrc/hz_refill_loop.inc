// The body of a refill kernel: included inside
//     template <bool COUNT, bool FAST> __global__ ... k_*_refill(Params ...)
// once `const ShadowParams &p` is in scope and the hooks below are defined.  Not a header: the hooks read and write the
// variables declared here (k_shadow_refill, k_accum_refill: hz_shadow.hip; k_viewshed_refill: hz_viewshed.hip;
// k_sight_refill: hz_sight.hip).
//
// A wave owns p.nb consecutive 8 x 8 blocks (the same quadrant of nb neighbouring 16 x 16 tiles) and hands their cells to
// its lanes as they become free.  The rays of one sun position are parallel, so with one ray per lane traced to completion
// (the round-2 kernel k_shadow, removed in round 6) a wave lasted as long as its longest ray while most lanes idled (45 % of
// the lanes active per VALU instruction, profiles/r02/pmc_shadow_summary.json); here a lane whose ray is finished takes the
// next cell once fewer than `regroup` lanes are still traversing (the ray compaction of the horizon kernel).  Cells are
// handed out in block order, so the rays in flight stay neighbours.
// FAST: the fast stack discipline of hz_trace (every pending sibling its own entry, written for the fewest instructions;
// `stack_cap` entries behind two padding rows).  A ray that runs out of entries is traced again, to completion, with the
// one-entry-per-level discipline in the same LDS column of its lane (the launcher makes sure the tree's height fits).
// COUNT: also count node visits / triangle tests / wave-level steps (Terrain count_work; the roofline's B_trav)
//
// Why an include and not a function template: k_shadow_refill<false, true> is one of the kernels whose device assembly
// stamps profiles/*.json (scripts/kernel_asm.py), so its machine code must not move.  With the loop in a __forceinline__
// template (the result step a lambda or an overload) the instruction counts stayed but register allocation and scheduling
// changed in every refill kernel -- even for k_shadow_refill's unchanged body merely wrapped in a function; with only the
// two hz_trace calls in a function the FAST instantiations grew by 4 - 17 instructions, and k_sight_refill's TAKE hook as a
// function moved its four instantiations.  As text all of them compile to the code they had as four copies
// (profiles/refill/asm_diff.txt), so the multi-line hooks stay macros.
//
// The hooks (every one must be defined, an empty definition where a kernel has nothing to do; all are #undef'd below):
//   HZ_REFILL_OUTPUTS         declarations: the kernel's outputs at position `pos` (HZ_REFILL_OUT_AT), other constants
//   HZ_REFILL_LANE            declarations: the lane's state, with the ray `r` (members ox, oy, oz, dx, dy, dz) hz_trace follows
//   HZ_REFILL_PASS            top of every pass of the loop, the whole wave is here
//   HZ_REFILL_BUSY            expression: the lane has a cell (its negation is the predicate of the hand-out)
//   HZ_REFILL_TAKE(i, j)      a free lane takes cell (i, j) of the inner domain: a ray starts (HZ_REFILL_START_RAY), or the
//                             cell is decided without one
//   HZ_REFILL_PREPARE         between hand-out and traversal
//   HZ_REFILL_TFAR, HZ_REFILL_TFAR_BOX   expressions: hz_trace's tfar and tfar_box of the lane's ray
//   HZ_REFILL_REGROUP         expression: hz_trace returns for a refill when fewer lanes than this still traverse
//   HZ_REFILL_DECIDED(res)    the lane's ray is decided (res: 1 hit, 0 none)
//   HZ_REFILL_END             after the loop, before the counters
#if !defined(HZ_REFILL_OUTPUTS) || !defined(HZ_REFILL_LANE) || !defined(HZ_REFILL_PASS) || !defined(HZ_REFILL_BUSY) || \
    !defined(HZ_REFILL_TAKE) || !defined(HZ_REFILL_PREPARE) || !defined(HZ_REFILL_TFAR) || !defined(HZ_REFILL_TFAR_BOX) || \
    !defined(HZ_REFILL_REGROUP) || !defined(HZ_REFILL_DECIDED) || !defined(HZ_REFILL_END)
#error "hz_refill_loop.inc: a kernel defines every HZ_REFILL_* hook before it includes the loop"
#endif
// an output of the launch (or null) at this workgroup's position
#define HZ_REFILL_OUT_AT(base) ((base) ? (base) + (size_t)pos * p.out_stride : nullptr)
// the lane's traversal starts over with the ray in R (box tests start at -tau and end at tfar + tau: hz_common.h)
#define HZ_REFILL_START_RAY(R) do { \
        rb = hz_raybox(((R).ox - p.sv.cx) - p.sv.tau * (R).dx, ((R).oy - p.sv.cy) - p.sv.tau * (R).dy, ((R).oz - p.sv.cz) - p.sv.tau * (R).dz, \
                       (R).dx, (R).dy, (R).dz); \
        hz_trav_reset(ts); \
        overflow = false; \
        rays++; } while (0)

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *stack = reinterpret_cast<int *>(smem + (FAST ? 2 * HZ_TPB * 4 : 0));
    const int tid = threadIdx.x;
    int ti = 0, tj = 0;
    const bool has_tile = hz_tile_of_block(p.tm, blockIdx.x, &ti, &tj);      // tile map over super tiles (16 x 16 nb cells)
    const int wave = tid >> 6, lane = tid & 63;
    const int pos = blockIdx.y;                     // the sun position / observer of the launch
    const float pos_x = p.suns[3 * pos], pos_y = p.suns[3 * pos + 1], pos_z = p.suns[3 * pos + 2];
    HZ_REFILL_OUTPUTS
    unsigned rays = 0;
    TravCounters tc; tc.nodes = 0; tc.tris = 0; tc.w_nodes = 0; tc.w_leaves = 0;
    const int i_base = ti * 16 + (wave >> 1) * 8, j_base = tj * (16 * p.nb) + (wave & 1) * 8;
    const int total = has_tile ? 64 * p.nb : 0;
    int next = 0;                                   // cells handed out so far (wave uniform)
    HZ_REFILL_LANE
    RayBox rb = hz_raybox(0, 0, 0, 0, 0, 1);
    TravState ts; hz_trav_reset(ts);
    bool overflow = false;
    for (;;) {
        HZ_REFILL_PASS
        if (next < total) {
            const unsigned long long need = __ballot(!(HZ_REFILL_BUSY));
            if (need != 0ull) {
                const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
                const int my = next + rank;
                next += __popcll(need);
                if (!(HZ_REFILL_BUSY) && my < total) {
                    const int i = i_base + ((my & 63) >> 3), j = j_base + (my >> 6) * 16 + (my & 7);
                    if (i < p.dim_in_0 && j < p.dim_in_1) {
                        HZ_REFILL_TAKE(i, j)
                    }
                }
            }
        }
        HZ_REFILL_PREPARE
        if (__ballot(HZ_REFILL_BUSY) == 0ull) {
            if (next >= total) break;
            continue;
        }
        if (HZ_REFILL_BUSY) {
            const float tfar = HZ_REFILL_TFAR, tfar_box = HZ_REFILL_TFAR_BOX;
            int res = hz_trace<HZ_TPB, COUNT, 2, false, !FAST>(p.sv.nodes, p.sv.prims, nullptr, 0, stack, tid, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz,
                                                    tfar, tfar_box, rb, ts, HZ_REFILL_REGROUP, HZ_SHADOW_LEAF_BIAS, tc, p.stack_cap, overflow);
            if (FAST && res != 2 && overflow) {
                bool unused = false;
                hz_trav_reset(ts);
                res = hz_trace<HZ_TPB, COUNT, 2, false, true>(p.sv.nodes, p.sv.prims, nullptr, 0, stack, tid, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz,
                                                                    tfar, tfar_box, rb, ts, 0, HZ_SHADOW_LEAF_BIAS, tc, 0, unused);
                if (COUNT && p.counters) atomicAdd(&p.counters[HZ_SHADOW_CNT_TWICE], 1ull);     // rays traced twice
            }
            if (res != 2) {
                HZ_REFILL_DECIDED(res)
            }
        }
    }
    HZ_REFILL_END
    shadow_counters<COUNT>(p, rays, tc, lane);

#undef HZ_REFILL_OUT_AT
#undef HZ_REFILL_START_RAY
#undef HZ_REFILL_OUTPUTS
#undef HZ_REFILL_LANE
#undef HZ_REFILL_PASS
#undef HZ_REFILL_BUSY
#undef HZ_REFILL_TAKE
#undef HZ_REFILL_PREPARE
#undef HZ_REFILL_TFAR
#undef HZ_REFILL_TFAR_BOX
#undef HZ_REFILL_REGROUP
#undef HZ_REFILL_DECIDED
#undef HZ_REFILL_END
