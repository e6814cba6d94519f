// ugp_dense.cpp -- the depth-first tables of a handle's tree (ugp_dense.hpp), built by the first attach of a handle and read by every
// query family, with the host helpers their attaches share: the same-arrays check, the leaf ranks and the stored alleles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "ugp_dense.hpp"

namespace ugp {

int dfs_tables_same_arrays(const DfsTables &T, const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const char *who) {
    const std::string other = std::string("the handle's depth-first tables were built from other mutation arrays (an earlier attach of this handle): ") +
                              who + " needs the arrays of that attach, or a handle of its own";
    const uint64_t M = tree->mut_off[tree->n_nodes];
    if (T.m != M || T.n != tree->n_nodes) return set_error(UGP_ERR_INVALID, other);
    if (hipSetDevice(T.device) != hipSuccess) return set_error(UGP_ERR_HIP, "hipSetDevice failed");
    std::vector<uint32_t> morig(M), mbits(M), moff((size_t)T.n + 1);
    std::vector<int32_t> mpos(M);
    UGP_HIP_TRY(hipMemcpy(moff.data(), T.moff.p, moff.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (M) {
        UGP_HIP_TRY(hipMemcpy(morig.data(), T.morig.p, M * sizeof(uint32_t), hipMemcpyDeviceToHost));
        UGP_HIP_TRY(hipMemcpy(mbits.data(), T.mbits.p, M * sizeof(uint32_t), hipMemcpyDeviceToHost));
        UGP_HIP_TRY(hipMemcpy(mpos.data(), T.mpos.p, M * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    uint64_t e = 0;
    bool same = true;
    for (uint64_t i = 0; i < T.n && same; i++) {
        const uint32_t b = dfs2bfs[i];
        same = moff[i] == e;   // the same entries on other nodes are other arrays: an entry moved to the next node keeps the flat order
        for (uint64_t k = tree->mut_off[b]; k < tree->mut_off[b + 1] && same; k++, e++)
            same = e < M && morig[e] == k && mpos[e] == tree->mut_pos[k] &&
                   (mbits[e] & 0xffffu) == ((uint32_t)tree->mut_nuc[k] | (uint32_t)tree->mut_ref[k] << 8);
    }
    if (!same || e != M) return set_error(UGP_ERR_INVALID, other);
    return UGP_OK;
}

void leaf_ranks(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, LeafRanks *out) {
    const uint32_t N = (uint32_t)dfs2bfs.size();
    std::vector<uint8_t> inner(N, 0);
    for (uint32_t j = 1; j < N; j++) inner[tree->parent[dfs2bfs[j]]] = 1;   // by BFS index
    out->leaf_dfs.clear();
    out->lbefore.resize((size_t)N + 1);
    for (uint32_t i = 0; i < N; i++) {
        out->lbefore[i] = (uint32_t)out->leaf_dfs.size();
        if (!inner[dfs2bfs[i]]) out->leaf_dfs.push_back(i);
    }
    out->lbefore[N] = (uint32_t)out->leaf_dfs.size();
    std::vector<uint32_t> sz(N, 1);   // subtree ends by a reverse sweep
    for (uint32_t i = N; i-- > 1;) sz[bfs2dfs[tree->parent[dfs2bfs[i]]]] += sz[i];
    out->dend.resize(N);
    for (uint32_t i = 0; i < N; i++) out->dend[i] = i + sz[i];
}

int stored_alleles(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const DfsTables &T, const char *who, std::vector<uint8_t> *mpn) {
    mpn->clear();
    mpn->reserve(T.m);
    for (uint32_t b : dfs2bfs)
        for (uint64_t e = tree->mut_off[b]; e < tree->mut_off[b + 1]; e++) {
            if (tree->mut_par[e] > 15 || tree->mut_nuc[e] > 15)
                return set_error(UGP_ERR_UNSUPPORTED, std::string(who) + ": entry " + std::to_string(e) + " has an allele above 15");
            mpn->push_back((uint8_t)(tree->mut_par[e] << 4 | tree->mut_nuc[e]));
        }
    if (mpn->size() != T.m) return set_error(UGP_ERR_INVALID, std::string(who) + ": the tables hold another number of entries");
    return UGP_OK;
}

int coded_alleles(const ugp_tree_desc *tree, const DfsTables &T, const std::string &needs) {
    if (T.m && !tree->mut_par) return set_error(UGP_ERR_INVALID, needs);
    for (uint64_t k = 0; k < T.m; k++) {
        if (tree->mut_pos[k] < 0) continue;
        if (tree->mut_nuc[k] < 1 || tree->mut_nuc[k] > 15 || tree->mut_par[k] < 1 || tree->mut_par[k] > 15)
            return set_error(UGP_ERR_UNSUPPORTED, "mut_nuc / mut_par of a non-masked mutation outside 1 .. 15");
    }
    return UGP_OK;
}

void dfs_tables_free(DfsTables *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

int dfs_tables(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               int entry_bits, DfsTables **tables) {
    if (!tree || !tables || !tree->parent || !tree->mut_off) return set_error(UGP_ERR_INVALID, "null argument");
    const uint64_t N = tree->n_nodes;
    if (N == 0 || N >= (1ull << 31) || dfs2bfs.size() != N || bfs2dfs.size() != N) return set_error(UGP_ERR_INVALID, "tree does not match the handle");
    const uint64_t M = tree->mut_off[N];
    if (M >= (1ull << entry_bits)) return set_error(UGP_ERR_UNSUPPORTED, "more than 2^" + std::to_string(entry_bits) + " mutation entries");
    if (M && (!tree->mut_pos || !tree->mut_ref || !tree->mut_nuc)) return set_error(UGP_ERR_INVALID, "null mutation arrays");
    if (*tables) return UGP_OK;
    try {
        std::unique_ptr<DfsTables> T(new DfsTables());
        T->device = device;
        T->n = (uint32_t)N;
        T->m = M;
        T->root_muts = (uint32_t)(tree->mut_off[1] - tree->mut_off[0]);
        T->bfs2dfs = bfs2dfs;
        std::vector<uint32_t> dpar(N), dend(N), depth(N), cum(N), moff(N + 1), mbits(M), mnode(M), mlink(M, kNil), morig(M);
        std::vector<int32_t> mpos(M), nrp(N, 0);
        std::vector<uint8_t> mflag(M, 0), leaf(N, 1);
        int32_t maxpos = -1;
        uint64_t e = 0;
        std::vector<int32_t> seen;   // positions of the current node's owners
        for (uint64_t i = 0; i < N; i++) {
            const uint32_t b = dfs2bfs[i];
            if (b >= N || bfs2dfs[b] != i) return set_error(UGP_ERR_INVALID, "depth-first order is not a permutation");
            dpar[i] = i ? bfs2dfs[tree->parent[b]] : kNil;
            if (i && dpar[i] >= i) return set_error(UGP_ERR_INVALID, "parent after child in depth-first order");
            moff[i] = (uint32_t)e;
            seen.clear();
            for (uint64_t k = tree->mut_off[b]; k < tree->mut_off[b + 1]; k++, e++) {
                const int32_t p = tree->mut_pos[k];
                mpos[e] = p;
                mbits[e] = (uint32_t)tree->mut_nuc[k] | (uint32_t)tree->mut_ref[k] << 8;
                mnode[e] = (uint32_t)i;
                morig[e] = (uint32_t)k;
                maxpos = std::max(maxpos, p);
                bool take = p < 0;
                if (p >= 0) {
                    if (std::find(seen.begin(), seen.end(), p) == seen.end()) { seen.push_back(p); take = true; mflag[e] |= kOwner; }
                    else T->literal_ok = false;
                }
                if (take && tree->mut_ref[k] != tree->mut_nuc[k]) mflag[e] |= kCounts;
            }
            depth[i] = i ? depth[dpar[i]] + 1 : 0;
            cum[i] = (i ? cum[dpar[i]] : 0) + (uint32_t)(tree->mut_off[b + 1] - tree->mut_off[b]);
            if (i) leaf[dpar[i]] = 0;
        }
        moff[N] = (uint32_t)e;
        if (maxpos >= (1 << 28)) return set_error(UGP_ERR_UNSUPPORTED, "mutation position above 2^28");
        // subtree ends: size by a reverse sweep
        {
            std::vector<uint32_t> sz(N, 1);
            for (uint64_t i = N; i-- > 1;) sz[dpar[i]] += sz[i];
            for (uint64_t i = 0; i < N; i++) dend[i] = (uint32_t)(i + sz[i]);
        }
        // owners by position, in depth-first order of their node; the nearest owning ancestor of each (a stack per position
        // whose top's subtree still contains the node) and its allele, the parent state
        const uint32_t tp = (uint32_t)(maxpos + 1);
        std::vector<uint32_t> poff(tp + 1, 0), pent;
        for (uint64_t k = 0; k < M; k++) if (mflag[k] & kOwner) poff[mpos[k] + 1]++;
        for (uint32_t p = 0; p < tp; p++) poff[p + 1] += poff[p];
        pent.resize(poff[tp]);
        {
            std::vector<uint32_t> fill(poff.begin(), poff.end() - 1);
            for (uint64_t k = 0; k < M; k++) if (mflag[k] & kOwner) pent[fill[mpos[k]]++] = (uint32_t)k;
        }
        std::vector<uint32_t> st;
        for (uint32_t p = 0; p < tp; p++) {
            st.clear();
            for (uint32_t x = poff[p]; x < poff[p + 1]; x++) {
                const uint32_t k = pent[x], u = mnode[k];
                while (!st.empty() && dend[mnode[st.back()]] <= u) st.pop_back();
                if (!st.empty()) {
                    const uint32_t a = st.back(), an = mbits[a] & 0xffu, ar = (mbits[a] >> 8) & 0xffu;
                    mbits[k] |= an << 16 | (uint32_t)(an != ar) << 24;
                    mlink[k] = a;
                }
                st.push_back(k);
            }
        }
        // nr(parent): positions off the reference on the parent's root path
        {
            std::vector<int32_t> nr(N, 0);
            for (uint64_t i = 0; i < N; i++) {
                int32_t v = i ? nr[dpar[i]] : 0;
                for (uint32_t k = moff[i]; k < moff[i + 1]; k++) {
                    if (!(mflag[k] & kOwner)) continue;
                    const uint32_t b = mbits[k];
                    v += ((b & 0xffu) != ((b >> 8) & 0xffu) ? 1 : 0) - (int32_t)((b >> 24) & 1u);
                }
                nr[i] = v;
                nrp[i] = i ? nr[dpar[i]] : 0;
            }
        }
        T->tp = tp;
        T->h_cum = cum;
        if (hipSetDevice(device) != hipSuccess) return set_error(UGP_ERR_HIP, "hipSetDevice failed");
        hipError_t err = hipSuccess;
        for (auto pr : {std::make_pair(&T->dpar, &dpar), std::make_pair(&T->dend, &dend), std::make_pair(&T->depth, &depth),
                        std::make_pair(&T->cum, &cum), std::make_pair(&T->moff, &moff), std::make_pair(&T->mbits, &mbits),
                        std::make_pair(&T->mnode, &mnode), std::make_pair(&T->mlink, &mlink), std::make_pair(&T->morig, &morig),
                        std::make_pair(&T->poff, &poff), std::make_pair(&T->pent, &pent)})
            if (err == hipSuccess) err = pr.first->upload(*pr.second);
        if (err == hipSuccess) err = T->mpos.upload(mpos);
        if (err == hipSuccess) err = T->nrp.upload(nrp);
        if (err == hipSuccess) err = T->mflag.upload(mflag);
        if (err == hipSuccess) err = T->leaf.upload(leaf);
        if (err != hipSuccess) return set_error(UGP_ERR_HIP, std::string("depth-first tables: ") + hipGetErrorString(err));
        *tables = T.release();
    } catch (const std::bad_alloc &) {
        return set_error(UGP_ERR_NOMEM, "out of host memory");
    }
    return UGP_OK;
}

}  // namespace ugp
