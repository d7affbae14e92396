// The leaf step of hz_trace (hz_common.h): included where the step stands in the traversal loop, once per control form of that
// loop.  Not a header: it reads and writes hz_trace's local variables.
            // ---------------- leaf step: the two triangles of a DEM quad (or one TIN triangle) ---
            if (LEND && !LEVELSTACK) {
                // 72 % of the lanes that test a leaf hold a second one (lq1) that would wait for another leaf step, while the
                // lanes without a leaf idle through this one.  Every lane of the loop tells its partner (lane ^ 1, one DPP move:
                // no LDS, no memory wait) what it holds: its second link (negative), "nothing queued" (HZ_EMPTY) or -- a lane
                // without a leaf -- 1 = "idle".  A partner outside the loop reads as 0: neither a link nor "idle".
                static_assert(HZ_EMPTY > 1, "the idle word must be neither a queued link (negative) nor HZ_EMPTY");
                // One block of straight VALU code for the exchange and the helper's operands: vcc = the lanes with a leaf;
                // w = can_leaf ? lq1 : 1; the ray a lane tests with = can_leaf ? its own : the partner's (v_cndmask_b32_dpp: the move
                // and its select in one instruction; a lane that is neither owner nor helper forms values nobody uses);
                // p_w = the partner's w (0 = the old value where the partner is outside the loop); lf = can_leaf ? lq0 : p_w.
                // Hazards, by hand (the compiler's hazard recogniser does not look inside an asm block): a DPP read of a VGPR needs
                // two wait states after the VALU write of it.  w (in lf) is written six instructions before v_mov_b32_dpp reads
                // it; ox ... dz are written at the refill only, outside this loop, and two instructions of the block come first.
                int p_w = 0, lf;
                float rox, roy, roz, rdx, rdy, rdz;
#define HZ_DPP_SEL(d, x) "v_cndmask_b32_dpp %[" d "], %[" x "], %[" x "], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                asm volatile("s_mov_b64 vcc, %[m]\n\t"
                             "v_cndmask_b32_e32 %[lf], 1, %[lq1], vcc\n\t"
                             HZ_DPP_SEL("rox", "ox") HZ_DPP_SEL("roy", "oy") HZ_DPP_SEL("roz", "oz")
                             HZ_DPP_SEL("rdx", "dx") HZ_DPP_SEL("rdy", "dy") HZ_DPP_SEL("rdz", "dz")
                             "v_mov_b32_dpp %[pw], %[lf] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                             "v_cndmask_b32_e32 %[lf], %[pw], %[lq0], vcc"
                             : [pw] "+&v"(p_w), [lf] "=&v"(lf), [rox] "=&v"(rox), [roy] "=&v"(roy), [roz] "=&v"(roz),
                               [rdx] "=&v"(rdx), [rdy] "=&v"(rdy), [rdz] "=&v"(rdz)
                             : [m] "s"(m_leaf), [lq0] "v"(lq0), [lq1] "v"(lq1), [ox] "v"(ox), [oy] "v"(oy), [oz] "v"(oz),
                               [dx] "v"(dx), [dy] "v"(dy), [dz] "v"(dz)
                             : "vcc");
#undef HZ_DPP_SEL
                const bool helper = !can_leaf && p_w < 0;                   // tests the partner's second leaf with the partner's ray
                const bool helped = can_leaf && lq1 < 0 && p_w == 1;        // this lane's second leaf is tested by the partner now
                if (COUNT && lcnt && can_leaf && lq1 < 0 && p_w != 1) lcnt->unhelped++;
                if (can_leaf || helper) {
                    float4 q0, q1, q2;
                    hz_load_prim(prims + HZ_LEAF_ID(lf), q0, q1, q2);
                    if (COUNT) { cnt.tris += (q2.y == q2.y) ? 2 : 1; HZ_WAVE_TICK(cnt.w_leaves, lane); if (lcnt && helper) lcnt->lent++; }
                    const bool hit = hz_quad_hit(rox, roy, roz, rdx, rdy, rdz, tfar, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                                 q2.x, q2.y, q2.z, q2.w, q2.y == q2.y);
                    // the helper's decision goes back the same way (only read by a lane whose partner is its helper, i.e. is here)
                    const int p_hit = __builtin_amdgcn_update_dpp(0, hit ? 1 : 0, 0xB1, 0xF, 0xF, true);
                    // owner: blocked by its own leaf, or by the lent one; else the queue moves up (the lent leaf is done with).
                    // A helper's own state does not change.
                    const bool lent_hit = helped && p_hit != 0;
                    const bool any = hit || lent_hit;
                    const int n_lq0 = any ? HZ_LEAF_ID(hit ? lq0 : lq1) : (helped ? HZ_EMPTY : lq1);
                    node = (can_leaf && any) ? HZ_EMPTY : node;
                    lq1 = (can_leaf && !any) ? HZ_EMPTY : lq1;
                    lq0 = can_leaf ? n_lq0 : lq0;
                }
            } else
            if (can_leaf) {
                float4 q0, q1, q2;
                hz_load_prim(prims + HZ_LEAF_ID(lq0), q0, q1, q2);
                // a = (q0.x q0.y q0.z) b = (q0.w q1.x q1.y) c = (q1.z q1.w q2.x) d = (q2.y q2.z q2.w)
                if (COUNT) { cnt.tris += (q2.y == q2.y) ? 2 : 1; HZ_WAVE_TICK(cnt.w_leaves, lane); }
                const bool hit = hz_quad_hit(ox, oy, oz, dx, dy, dz, tfar, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                             q2.x, q2.y, q2.z, q2.w, q2.y == q2.y);
                if (hit) { lq0 = HZ_LEAF_ID(lq0); node = HZ_EMPTY; }     // decided: blocked by this leaf
                else { lq0 = lq1; lq1 = HZ_EMPTY; }
            }
