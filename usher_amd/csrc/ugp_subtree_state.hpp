// ugp_subtree_state.hpp -- the state behind ugp_subtree_attach, shared by the single call (ugp_subtree.hip) and the batched call
// (ugp_subtree_batch.hip).  Only those two files include it.
#pragma once
#include "ugp_dense.hpp"

namespace ugp {

struct BatState;                // the batched call's workspace and last result (ugp_subtree_batch.hip), made by its first call
void bat_free(BatState *b);

struct SubState {
    int device = 0;
    hipStream_t stream = nullptr;
    const DfsTables *T = nullptr;                 // the handle's
    const std::vector<uint32_t> *dfs2bfs = nullptr;
    DBuf<uint8_t> mpn;                            // per depth-first entry: stored parent allele << 4 | allele
    DBuf<uint32_t> at, seg, sb, kb, kdfs, kpar, eb, vin, vout, sv, sfirst, ofirst, eoff, qat, qown;
    DBuf<uint8_t> sel, kept, eflag, surv, snuc, onuc;
    DBuf<unsigned long long> kin, kout, ctr;
    DBuf<int32_t> opos;
    DBuf<unsigned char> tmp;
    bool have = false;                            // the buffers hold a selection's answer
    uint32_t nk = 0, G = 0, E = 0;                // kept nodes, gathered entries, merged entries
    BatState *bat = nullptr;
    ~SubState() {
        bat_free(bat);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace ugp
