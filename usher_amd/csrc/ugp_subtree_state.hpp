// ugp_subtree_state.hpp -- the state behind ugp_subtree_attach, shared by the single call (ugp_subtree.hip) and the batched call
// (ugp_subtree_batch.hip).  Only those two files include it.
#pragma once
#include "ugp_query.hpp"

namespace ugp {

struct BatState;                // the batched call's workspace and last result (ugp_subtree_batch.hip), made by its first call
void bat_free(BatState *b);

struct SubState : QueryBase {
    DBuf<uint8_t> mpn;                            // per depth-first entry: stored parent allele << 4 | allele
    DBuf<uint32_t> at, seg, sb, kb, kdfs, kpar, eb, vin, vout, sv, sfirst, ofirst, eoff, qat, qown;
    DBuf<uint8_t> sel, kept, eflag, surv, snuc, onuc;
    DBuf<unsigned long long> kin, kout, ctr;
    DBuf<int32_t> opos;
    DBuf<unsigned char> tmp;
    bool have = false;                            // the buffers hold a selection's answer
    uint32_t nk = 0, G = 0, E = 0;                // kept nodes, gathered entries, merged entries
    BatState *bat = nullptr;
    ~SubState() { bat_free(bat); }
};

// The run of the sorted items that starts at i (the entries val[j] for j from i while j < G and key[j] == k, top-down) through
// add_mutation's states.  True when an entry survives: *first is then the run's first entry since the position was last empty and *sn
// the surviving allele.  *bad counts the entries add_mutation refuses.
__device__ __forceinline__ bool walk_run(uint32_t i, uint32_t G, unsigned long long k, const unsigned long long *key, const uint32_t *val,
                                         const uint8_t *mpn, uint32_t *first_out, uint32_t *sn_out, uint32_t *bad_out) {
    bool open = false;
    uint32_t first = 0, spar = 0, sn = 0, bad = 0;
    for (uint32_t j = i; j < G && key[j] == k; j++) {
        const uint32_t e = val[j], par = mpn[e] >> 4, nuc = mpn[e] & 15u;
        if (!open) { open = true; first = e; spar = par; sn = nuc; }   // nothing is checked, par == nuc included
        else if (spar != nuc) sn = nuc;
        else if (sn == par) open = false;                               // a reversal empties the position
        else bad++;                                                     // add_mutation's false: the entry is skipped
    }
    *first_out = first; *sn_out = sn; *bad_out = bad;
    return open;
}

}  // namespace ugp
