// The node step of hz_trace (hz_common.h), for the lanes with a node: included where the step stands in the traversal loop, once per
// control form of that loop.  Not a header: it reads and writes hz_trace's local variables.
                float4 n0; uint4 n1;
                // NODELET: top-of-tree nodes from LDS, the rest from global memory (two separate asm paths:
                // a per-lane pointer select would be compiled into slow flat loads).  Measured 2 % slower
                // than plain global loads -- the top of the tree is L1 resident -- so it is opt-in.
                if (NODELET && node < ntop) hz_load_node_lds(top + 2 * node, n0, n1);
                else if (LEAN) hz_load_node(nodes + (unsigned)node, n0, n1);      // (no sign extension; v_lshl_add_u64 shifts by 4 at most: two instructions)
                else hz_load_node(nodes + node, n0, n1);
                if (COUNT) { cnt.nodes++; HZ_WAVE_TICK(cnt.w_nodes, lane); }
                const NodeRay nr = hz_node_ray(rb, n0.x, n0.y, n0.z);
                // children are visited in slot order (quadrant order).  A front-to-back order (slot r ^ direction
                // signs, ~45 VALU per step) was measured to be a net loss: these are any-hit rays, a blocked ray
                // is blocked over a long stretch behind the first ridge, and near-horizon rays that only
                // nick a crest are served by the hit cache.  (Rounds 2-3 stored the tallest child first: +1 %; the
                // quadrant order is what lets x and y share one range per half, i.e. the 32 B node.)
                const int first = __float_as_int(n0.w);
                if (LEVELSTACK) {
                    bool h0, h1, h2, h3;
                    hz_node_hits(nr, rb, tfar_box, n1, h0, h1, h2, h3);
                    const int h = (h0 ? 1 : 0) | (h1 ? 2 : 0) | (h2 ? 4 : 0) | (h3 ? 8 : 0);
                    if (h != 0) {                    // the hit children become the pending set of this level ...
                        if (pm != 0) { stack[sp * TPB + tid] = hz_entry_pack(pf, pm); sp++; }
                        pf = first; pm = h;
                    }
                    HZ_POP();                        // ... and the first of them (or of a level above) is entered
                } else {
                    int m0, m1, m2, m3;              // lane masks: all ones = child hit (hz_node_hit_masks)
                    if (LEAN) hz_node_hit_masks_t<true>(nr, rb, sel_x1, sel_y1, tfar_box, n1, m0, m1, m2, m3);
                    else hz_node_hit_masks(nr, rb, tfar_box, n1, m0, m1, m2, m3);
                    // out of entries: remember the highest pointer (checked once, at the exit) and clamp
                    sa_hi = max(sa_hi, sa);
                    sa = min(sa, sa_cap);
                    // Pushes without a branch, without scalar logic and (round 5) without compares: the three candidates are
                    // always stored above the top and only kept (pointer advanced) when they were real links, i.e. when a
                    // higher slot was hit too.  The hit masks become 0 / one-entry steps (a_k = m_k & S), "a higher slot was
                    // hit" is an OR of those, "advance" an AND; the link that continues is picked with bit selects (m ? x : y
                    // = v_bfi_b32); the lane without a hit child continues with the top entry pv and steps down.
                    const unsigned S = (unsigned)(TPB * 4);
                    const int pv = HZ_STACK_AT(sa + S);
                    const unsigned a0 = (unsigned)m0 & S, a1 = (unsigned)m1 & S, a2 = (unsigned)m2 & S, a3 = (unsigned)m3 & S;
                    const unsigned o32 = a3 | a2, o321 = o32 | a1, o3210 = o321 | a0;
#define HZ_SEL(m, x, y) (((m) & (x)) | (~(m) & (y)))
                    int next = HZ_SEL(m3, first + 3, pv);
                    HZ_STACK_AT(sa + 2u * S) = next; sa += a2 & a3;   next = HZ_SEL(m2, first + 2, next);
                    HZ_STACK_AT(sa + 2u * S) = next; sa += a1 & o32;  next = HZ_SEL(m1, first + 1, next);
                    HZ_STACK_AT(sa + 2u * S) = next; sa += a0 & o321; next = HZ_SEL(m0, first, next);
#undef HZ_SEL
                    node = next; sa = sa + o3210 - S;
                }
