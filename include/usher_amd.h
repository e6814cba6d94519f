/*
 * usher_amd.h -- C ABI of the MI355X placement engine (libusher_amd.so).
 *
 * Drop-in boundary for UShER's parsimony-placement hot path.  The reference
 * has no FFI layer: the seam is the C++ call
 *     void mapper2_body(mapper2_input&, bool, bool)      src/usher_graph.hpp:103
 * made N times per sample from three tbb::parallel_for blocks in
 * usher_common()                                         src/usher_common.cpp:252-273, 389-414, 426-449
 * (4 more call sites in matUtils / ripples).  This library replaces the whole
 * per-sample block (usher_common.cpp:342-449) for a BATCH of samples against a
 * static tree: the caller hands over the tree once (ugp_mat_create), then any
 * number of query batches (ugp_place_batch & friends).  Plain pointers and
 * sizes only; no C++ or torch types cross the boundary; nothing is thrown and
 * the process is never exited (the reference's loaders call exit(1),
 * mutation_annotated_tree.cpp:473-475, 894-896, 2142-2145).
 *
 * Node numbering.  Every node index in this API is the node's position in the
 * reference's breadth-first expansion (Tree::breadth_first_expansion,
 * mutation_annotated_tree.cpp:1225-1251) -- the `j` of usher_common.cpp:391-403
 * and mapper2_input::j (usher_graph.hpp:82).  Tie-breaking among equally
 * parsimonious nodes (usher_mapper.cpp:483-486) is by larger number of
 * descendant leaves, then larger j, exactly as the reference.
 *
 * Alleles are the reference's one-hot codes A=1 C=2 G=4 T=8, ambiguity codes
 * are unions, N = 15 (mutation_annotated_tree.cpp:19-74).
 */
#ifndef USHER_AMD_H
#define USHER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UGP_OK               0
#define UGP_ERR_INVALID     -1   /* bad argument / malformed tree or query arrays            */
#define UGP_ERR_UNSUPPORTED -2   /* input violates a precondition of the device algorithm    */
#define UGP_ERR_HIP         -3   /* a HIP runtime call failed (no device, out of memory ...)  */
#define UGP_ERR_NOMEM       -4   /* host allocation failed                                    */

/* Opaque handle: the flattened mutation-annotated tree resident in the HBM of
 * one device (replaces MAT::Tree* + the BFS vector of usher_common.cpp:342).
 * Threading: a handle owns its per-call workspaces, so calls on ONE handle must come from one thread at a time (the
 * reference serialises samples behind its global locks the same way, usher_mapper.cpp:3-4); different handles -- on the
 * same or on different devices -- are independent and may be driven by different host threads.  Overlap of batches on one
 * handle is what ugp_place_device / ugp_place_batch_async are for.  ugp_last_error() is per thread. */
typedef struct ugp_mat ugp_mat;
/* Opaque handle: a validated query batch resident in HBM. */
typedef struct ugp_qset ugp_qset;

/*
 * The tree, as flat arrays in BFS order (replaces MAT::Node / MAT::Mutation,
 * mutation_annotated_tree.hpp:45-111).  Children of a node are the nodes that
 * name it as parent, in increasing index (= the reference's child order).
 */
typedef struct ugp_tree_desc {
    uint64_t n_nodes;
    const uint32_t *parent;   /* [n_nodes]   parent[0] = UINT32_MAX, parent[j] < j            */
    const uint64_t *mut_off;  /* [n_nodes+1] CSR offsets into the mutation arrays             */
    const int32_t *mut_pos;   /* [n_muts]    1-based position; < 0 = masked (hpp:76-78)       */
    const uint8_t *mut_ref;   /* [n_muts]    one-hot reference base (ignored when masked)     */
    const uint8_t *mut_par;   /* [n_muts]    parent allele as stored in the MAT (informational:
                                             the library derives the true parent state itself,
                                             like usher_mapper.cpp:275-286 does)              */
    const uint8_t *mut_nuc;   /* [n_muts]    one-hot mutated base                             */
} ugp_tree_desc;

/*
 * A batch of query samples: per sample the rows read_vcf() would have put in
 * Missing_Sample::mutations (mutation_annotated_tree.cpp:2234-2270,
 * usher_graph.hpp:33-53).  Rows of one sample must be sorted by position with
 * no duplicates (UGP_ERR_UNSUPPORTED otherwise).
 */
typedef struct ugp_queries {
    uint64_t n_queries;
    const uint64_t *ent_off;     /* [n_queries+1] CSR offsets                                  */
    const int32_t *pos;          /* [n_ent] position                                           */
    const uint8_t *ref;          /* [n_ent] one-hot VCF REF base                               */
    const uint8_t *nuc;          /* [n_ent] allele mask of the sample at pos (15 when missing) */
    const uint8_t *is_missing;   /* [n_ent] 1 for N / '.' cells (mutation.is_missing)          */
} ugp_queries;

/* Per-sample placement summary: the values usher_common.cpp:451-453 prints and
 * uses -- *best_set_difference, *num_best, *best_j, *has_unique of
 * mapper2_input (usher_graph.hpp:79-92). */
typedef struct ugp_result {
    int32_t best_set_difference;   /* parsimony score of the best placement            */
    uint32_t num_best;             /* number of equally parsimonious placements        */
    uint32_t best_j;               /* BFS index of the chosen node                     */
    uint32_t best_has_unique;      /* 1: place as sibling even if the node is internal */
} ugp_result;

typedef struct ugp_info {
    uint64_t n_nodes;
    uint64_t n_muts;            /* non-masked mutations                                        */
    uint64_t n_sites;           /* distinct mutated positions (rows of an allele tile)         */
    uint64_t stream_bytes;      /* device bytes of the DFS record stream read per tree pass    */
    uint64_t algo_tree_bytes;   /* 4*M + 8*N                                      */
    uint64_t algo_tile_bytes;   /* per sample, L/2 + 16                           */
    uint32_t n_chunks;
    uint32_t max_slots;         /* depth of the per-lane D stack the tree needs                */
    uint32_t max_position;
    uint32_t device;
} ugp_info;

typedef struct ugp_timing {
    float table_ms;      /* allele-tile build kernels of the last call          */
    float place_ms;      /* the dominant kernel of the last call (k_best8, or k_place on the 32-bit path) */
    float merge_ms;      /* reduction after it (phase 2: k_gbest/k_select/k_ties/k_final, or k_merge)     */
    uint32_t place_launches;
    uint32_t n_tiles;    /* sample tiles (one tree pass each) in the last call: 512-sample tiles on
                            the packed path, 64-sample tiles on the 32-bit path */
    uint32_t n_groups;   /* waves per tile in the last call                     */
    uint32_t packed_path; /* 1: 8-samples-per-lane 16-bit kernel + phase 2; 0: 32-bit kernel */
    uint32_t reserved;
    uint64_t words_total;   /* packed path: stream words x tiles the dominant kernel had to cover      */
    uint64_t words_skipped; /* ... of which exact lower-bound pruning skipped (0 with UGP_NO_PRUNE)    */
    float coarse_ms;     /* locality pre-pass of the last call (placement on the coarse top-of-tree MAT), 0 when not run */
    uint32_t bound3;     /* 1: the last call's main walk used the third pruning bound (its per-batch tables were built); ugp_get_timing_sum: how many calls did */
} ugp_timing;

/* Optional: bring up the HIP runtime and the context of `device` now (what the first ugp_mat_create on that device would pay: a few
 * tenths of a second) -- e.g. on a thread of its own while the caller is still reading its inputs.  Thread-safe; calling it again, or
 * never, is harmless. */
int ugp_device_warmup(int device);

/* Flatten + upload.  device = HIP device ordinal.  Replaces the per-sample
 * BFS rebuild and 2N vector allocations of usher_common.cpp:342-365. */
int ugp_mat_create(const ugp_tree_desc *tree, int device, ugp_mat **out);
/* Same tree on several devices of one node (flattened once, uploaded n times): the replicated read-only MAT of
 * the multi-GPU path -- query samples shard across the handles, one host thread per handle. */
int ugp_mat_create_multi(const ugp_tree_desc *tree, const int *devices, int n_devices, ugp_mat **out /* [n_devices] */);
/* One process per GPU (the ranks of a torch.distributed / MPI launch): the flattening is host work with the same result on every
 * rank.  ugp_flat_save runs it once and writes the result to `path` (put it on /dev/shm: a memory copy of ~0.6 GB at 10M nodes);
 * ugp_mat_create_from_flat uploads that file to `device` without flattening again.  The file is only valid for the library build
 * and the flattening switches (UGP_CHUNK_NODES ...) it was written under -- checked, UGP_ERR_UNSUPPORTED otherwise. */
int ugp_flat_save(const ugp_tree_desc *tree, const char *path);
int ugp_mat_create_from_flat(const char *path, int device, ugp_mat **out);
void ugp_mat_destroy(ugp_mat *mat);
int ugp_mat_info(const ugp_mat *mat, ugp_info *out);

/*
 * Score every node of the tree for every query sample and reduce to the best
 * placement: passes 1 and 2 of usher_common.cpp:389-449 for each sample (static
 * tree: the -n / -p semantics).  Host buffers in, host buffer out, synchronous.
 */
int ugp_place_batch(ugp_mat *mat, const ugp_queries *q, ugp_result *out /* [n_queries] */);

/*
 * -p / --write-parsimony-scores-per-node (usher_common.cpp:406-412, 557-578):
 * out[q * n_nodes + j] = set_difference of placing sample q at BFS node j, +1
 * when the node is not an eligible placement (usher_mapper.cpp:498-502).
 */
int ugp_scores_per_node(ugp_mat *mat, const ugp_queries *q, int32_t *out /* [n_queries * n_nodes] */);

/*
 * best_j_vec / node_has_unique (usher_graph.hpp:89-90): all equally
 * parsimonious nodes of each sample, ascending BFS index (the order
 * usher_common.cpp:588 sorts them into), at most `cap` per sample;
 * tie_count[q] receives the true count.
 */
int ugp_tied_nodes(ugp_mat *mat, const ugp_queries *q, uint32_t cap,
                   uint32_t *tie_j /* [n_queries * cap] */,
                   uint8_t *tie_has_unique /* [n_queries * cap] */,
                   uint32_t *tie_count /* [n_queries] */);

/* ---- the other callers of mapper2_body ------------------------------------------------------------------
 * matUtils uncertainty (uncertainty.cpp:212-235: every node but the sample's own, depth-first indices), annotate
 * (annotate.cpp:615-638: depth-first indices; rows it cannot take: ugp_annotate_search), merge (merge.cpp:253-280: the breadth-first expansion of a subtree, cut
 * max_levels below its root) and ripples (ripples/main.cpp:343-377: nodes with enough descendants, a per-node
 * distance, per-node scores) run the same search over THEIR node vector: the index j they hand to mapper2_body --
 * which also breaks ties, usher_mapper.cpp:483-486 -- is a position in that vector.  These entry points take the
 * vector as an order (breadth-first or the reference's depth-first expansion, mutation_annotated_tree.cpp:1253-1273)
 * plus a mask; every node index going in or out is a position in the chosen order.  (A breadth-first expansion of a
 * subtree lists its nodes in the same relative order as the whole tree's, so merge's sub-BFS is order BFS + mask.)
 * Exact for any combination of options.  An order, a distance, a mask and an excluded node per sample run on the packed,
 * pruned path of ugp_place_batch (the order / distance is the tie rank of its second phase, the mask a temporary "no
 * candidate" bit in the tree on the device, the excluded node is taken out of the one chunk minimum it may have set);
 * the score matrix of a breadth-first search comes from the level-by-level kernel of ugp_scores_per_node; the score matrix in
 * depth-first indices and a mask that drops the root take the general one-sample-per-lane kernel (no pruning). */
#define UGP_ORDER_BFS 0u
#define UGP_ORDER_DFS 1u
typedef struct ugp_place_opts {
    uint32_t order;              /* UGP_ORDER_BFS / UGP_ORDER_DFS: meaning of every node index of this call             */
    const uint8_t *node_mask;    /* [n_nodes] or NULL: 0 = the node is not scored (shared by all samples of the call)   */
    const uint32_t *skip_node;   /* [n_queries] or NULL: one node left out for that sample, UINT32_MAX = none           */
    const uint32_t *distance;    /* [n_nodes] or NULL: mapper2_input::distance; among equal scores the smaller wins     */
    int32_t *scores;             /* [n_queries * n_nodes] or NULL: per-node scores as compute_parsimony_scores = true
                                    reports them (+1 when not eligible); nodes that were not scored read 0             */
} ugp_place_opts;
/* If no admitted node is eligible the result is {INT32_MAX, 0, UINT32_MAX, 0} (the reference's callers would be left
 * with their initial values). */
int ugp_place_batch_ex(ugp_mat *mat, const ugp_queries *q, const ugp_place_opts *opts, ugp_result *out /* [n_queries] */);
int ugp_tied_nodes_ex(ugp_mat *mat, const ugp_queries *q, const ugp_place_opts *opts, uint32_t cap, uint32_t *tie_j,
                      uint8_t *tie_has_unique, uint32_t *tie_count);
/* The node-level options prepared once.  ripples (ripples/main.cpp:303-377) runs thousands of searches with ONE node vector -- the
 * nodes with enough descendant leaves -- and ONE distance array; remapping a 10M-entry mask, ranking 10M (distance, leaves) keys and
 * uploading both is then the call (40 of 43 ms per 4,096 samples at 10M nodes).  ugp_ex_prepare does that part once: `opts`
 * contributes order, node_mask and distance (both copied: the arrays may be freed), its skip_node / scores are ignored.  The handle
 * belongs to `mat` and must be destroyed before it.
 * ugp_place_batch_prepared = ugp_place_batch_ex with those options plus, per call, skip_node ([n_queries] positions in the prepared
 * order, or NULL) and d_scores: a DEVICE buffer of n_queries * n_nodes int32 (or NULL) that receives the score matrix as
 * ugp_place_opts::scores describes it -- written by the level-by-level kernel of ugp_scores_per_node for a breadth-first order (no
 * host copy: a caller that reduces the rows on the device, as ripples' per-node filter could, never moves the 40 MB per sample),
 * valid when the call returns. */
typedef struct ugp_ex ugp_ex;
int ugp_ex_prepare(ugp_mat *mat, const ugp_place_opts *opts, ugp_ex **out);
void ugp_ex_destroy(ugp_ex *ex);
int ugp_place_batch_prepared(ugp_mat *mat, const ugp_queries *q, const ugp_ex *ex, const uint32_t *skip_node, ugp_result *out /* [n_queries], host */,
                             int32_t *d_scores /* device, or NULL */);
/* matUtils uncertainty (uncertainty.cpp:132-339): for each node S of `nodes` (breadth-first indices) the search findEPPs runs --
 * the sample is S's root path in the reference's LITERAL order (S's own mutations, then each ancestor's, most recent per position,
 * masked entries kept, not sorted), every node but S is scored in the depth-first expansion, the initial best is |Q| + |root
 * mutations| + 1 with best_j_vec = {0} -- and its results:
 *   epps[i]      = num_best (equally parsimonious placements); 0 when Q(S) is empty (the reference skips the search and prints
 *                  uninitialised values there, uncertainty.cpp:167, 326-333);
 *   tie_count[i] = the true size of the tie set (= epps[i]); tie_dfs[i * cap ..] its first min(cap, tie_count[i]) depth-first
 *                  positions, ascending (the reference appends in TBB's order; a serial run's order is fixed here);
 *   nsize[i]     = get_neighborhood_size (:41-130) over the WHOLE tie set when num_best > 1, else 0 -- never depends on cap.
 * Every pair is scored (dense; exact for the literal row order, which ugp_place_batch_ex cannot take).  The tables come from
 * ugp_uncertainty_attach, once per handle: `tree` must be the tree the handle was created from (same parent array; the arrays
 * are copied and may be freed).  A tree with two non-masked mutations at one position on one branch is UGP_ERR_UNSUPPORTED.
 * The handle's depth-first tables are shared as ugp_genotypes_attach describes: when another attach has built them, `tree` must
 * carry the mutation arrays of that attach (UGP_ERR_INVALID otherwise, nothing changed).  A later attach replaces the tables. */
int ugp_uncertainty_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_uncertainty(ugp_mat *mat, const uint32_t *nodes /* BFS */, uint64_t n, uint32_t cap, uint32_t *epps, uint32_t *nsize,
                    uint32_t *tie_dfs /* [n * cap] */, uint32_t *tie_count);
/* matUtils annotate (annotate.cpp:301-419, 466-481, 611-638).  ugp_annotate_attach makes the depth-first tables of `tree` once per
 * handle (the handle's tree: same parent array; arrays are copied); they are shared as ugp_genotypes_attach describes: when
 * another attach has built them, `tree` must carry the mutation arrays of that attach (UGP_ERR_INVALID otherwise, nothing
 * changed).  Clades are CSR lists of exemplar nodes (BFS indices); an exemplar listed twice counts twice, as in the reference.
 * ugp_clade_alleles: for each clade, every mutation entry (its index in tree->mut_off's CSR) that the reference's walk
 *   rsearch(exemplar, true) adds (:355-390) -- the first non-masked entry of a position wins (later ones on the same node and
 *   older ones above are skipped), masked entries always count, entries with ref == mut count nothing -- and how many of the
 *   clade's exemplars add it.  Entries come per clade (out_off[c] .. out_off[c + 1]) in depth-first order of their node, then
 *   stored order; only entries with a count > 0 are listed.  out_ent / out_cnt receive the first min(cap, *n_out) of them and
 *   *n_out the true total; out_off [n_clades + 1] is always written.
 * ugp_clade_descendants: out[i] = exemplars of clade pair_clade[i] strictly below node pair_node[i] (BFS): is_ancestor
 *   (mutation_annotated_tree.cpp:920-929) starts at the parent, so a node is not its own descendant.
 * ugp_annotate_search: annotate's search (:611-638) literally, for any rows -- repeated positions and masked (negative) positions
 *   included, which ugp_place_batch_ex refuses: mapper2_body over every node of the depth-first expansion in the rows' stored
 *   order, best = 1e9.  Per query: best[s] = the best score, tie_count[s] = the number of tied nodes, tie_dfs[s * cap ..] the
 *   first min(cap, tie_count[s]) of them as depth-first positions, ascending.  Rows must have is_missing = 0 (UGP_ERR_INVALID);
 *   a tree with two non-masked mutations at one position on one branch is UGP_ERR_UNSUPPORTED here.  Queries run one at a time:
 *   when a later query fails its checks, the earlier queries' outputs are already written. */
int ugp_annotate_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_clade_alleles(ugp_mat *mat, const uint64_t *clade_off /* [n_clades + 1] */, const uint32_t *nodes /* BFS */, uint64_t n_clades,
                      uint64_t *out_off /* [n_clades + 1] */, uint32_t *out_ent, uint32_t *out_cnt, uint64_t cap, uint64_t *n_out);
int ugp_clade_descendants(ugp_mat *mat, const uint64_t *clade_off, const uint32_t *nodes /* BFS */, uint64_t n_clades,
                          const uint32_t *pair_clade, const uint32_t *pair_node /* BFS */, uint64_t n_pairs, uint32_t *out);
int ugp_annotate_search(ugp_mat *mat, const ugp_queries *q, uint32_t cap, int32_t *best /* [n_queries] */, uint32_t *tie_dfs /* [n_queries * cap] */,
                        uint32_t *tie_count /* [n_queries] */);
/* matUtils extract's "k nearest samples" (get_nearby, matUtils/select.cpp:206-276) for a batch of queries.  ugp_nearest_attach makes
 * the depth-first tables of `tree` (the handle's tree: same parent array; arrays are copied) and a leaf prefix table, once per handle.
 * The depth-first tables are shared as ugp_genotypes_attach describes: when another attach has built them, `tree` must carry the
 * mutation arrays of that attach (UGP_ERR_INVALID otherwise, nothing changed).
 * ugp_nearest_k: query i is a node (BFS index; any node, not only a leaf) and its own k[i] > 0.  As the reference: climbing from the
 * node itself, last_anc is the last ancestor with <= k leaves (the node to begin with) and anc the first with more; the result is
 * the leaves of last_anc in depth-first order, then the leaves under anc that are not strict descendants of last_anc (is_ancestor
 * starts at the parent: a leaf last_anc is a candidate of its own search and may be listed twice, as in the reference), ascending by
 * the number of mutation entries -- masked ones included -- between the leaf and anc, until k are held.  Two rules follow from
 * the reference's loop and are kept: NO ancestor with more than k leaves -> an EMPTY result (count 0, anc UINT32_MAX); a node
 * with more than k leaves of its own -> anc == last_anc == the node and ALL its leaves (count > k; the first min(count,
 * out_stride) are written).  One deviation: the reference orders equal distances by whatever its unstable std::sort leaves; here
 * ties come in depth-first order (a stable sort).  The reference's set is therefore unique only when n_at_cut equals the number
 * of entries at distance cut_dist in the result.
 * Row i of out_nodes (BFS indices) / out_dist (distance to anc) has out_stride slots, the first min(count, out_stride) written;
 * out_stride >= the largest k.  An out-of-range node, k = 0 or a smaller out_stride is UGP_ERR_INVALID before anything is written.
 * Queries run in chunks of bounded device workspace; ugp_nearest_k_chunked (test hook) sets the queries per chunk (0: default). */
typedef struct ugp_nearest_info {
    uint32_t count;      /* size of the reference's result                                                        */
    uint32_t anc;        /* BFS index of the first ancestor with more than k leaves; UINT32_MAX: none             */
    uint32_t last_anc;   /* BFS index of the last ancestor with at most k leaves                                  */
    uint32_t cut_dist;   /* d*: the largest distance among the candidates taken (0 when none is taken)            */
    uint32_t n_at_cut;   /* candidates at distance d* (0 when none is taken)                                      */
} ugp_nearest_info;
int ugp_nearest_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_nearest_k(ugp_mat *mat, uint64_t n_queries, const uint32_t *nodes /* BFS */, const uint32_t *k, uint32_t out_stride,
                  uint32_t *out_nodes /* [n_queries * out_stride] */, uint32_t *out_dist /* [n_queries * out_stride] */,
                  ugp_nearest_info *info /* [n_queries] */);
int ugp_nearest_k_chunked(ugp_mat *mat, uint64_t n_queries, const uint32_t *nodes, const uint32_t *k, uint32_t out_stride,
                          uint32_t *out_nodes, uint32_t *out_dist, ugp_nearest_info *info, uint32_t chunk_queries);
/* matUtils extract -v (make_vcf / r_add_genotypes, matUtils/convert.cpp:53-292): the VCF site table and genotype codes of a selection
 * of nodes.  ugp_genotypes_attach shares the depth-first tables of `tree` (the handle's tree; arrays are copied; mut_par is needed,
 * and mut_nuc / mut_par of non-masked mutations must lie in 1 .. 15, UGP_ERR_UNSUPPORTED otherwise), once per handle.
 * The handle's depth-first tables are shared by every dense attach (uncertainty, annotate, nearest, relatives, select, mask, subtree,
 * genotypes, summary, translate, haplotypes) and are built by the first of them: when they exist, EVERY one of these attaches checks
 * that `tree` carries the mutation arrays they were built from (compared entry by entry; UGP_ERR_INVALID otherwise, nothing
 * changed) -- a handle takes one set of mutation arrays for its whole life.
 * ugp_genotype_select: the selection is a set of nodes (BFS indices; any node; one given twice counts once; NULL or n = 0: all
 * leaves).  Columns are the selected nodes in depth-first order.  Masked mutations (mut_pos < 0) are skipped everywhere.  At a
 * position p a column is COVERED when a node of its root path (itself included) has a mutation at p; its allele is mut_nuc of the
 * deepest such node (the last stored one when that node has several at p).  REF is mut_par AS STORED of the first stored mutation
 * at p of the first node, in depth-first order, that has one and a selected node in its subtree.  The alternates are the distinct
 * alleles != REF of the covered columns in ascending numeric order of their 4-bit code (ambiguous codes are alleles like any
 * other); ac[] counts their columns, AN is n_cols.  A position where no column is covered, or every covered column carries REF, is
 * no site.  Sites come in ascending position.  A genotype code is 0 for an uncovered column or REF, else 1 + the index of the
 * allele in alt[].  The selection, its counts and the site table stay on the device until the next select of the handle.
 * ugp_genotype_columns: the columns' nodes.  ugp_genotype_sites: rows [lo, hi) of the site table.  ugp_genotype_rows: the codes of
 * sites [lo, hi), row-major with stride n_cols; they are computed in windows of bounded device workspace, and
 * ugp_genotype_rows_chunked (test hook) sets the cells per window (0: default; a window smaller than a row is a part of one row,
 * in steps of 16 columns).  An out-of-range node, lo > hi, hi > n_sites, or sites / rows / columns before a select are
 * UGP_ERR_INVALID before anything is written. */
typedef struct ugp_gt_site {
    int32_t pos;
    uint8_t ref, n_alt;
    uint8_t alt[14];     /* ascending 4-bit codes                                  */
    uint32_t ac[14];     /* covered columns with alt[k]                            */
    uint32_t covered;    /* covered columns (those with REF included)              */
} ugp_gt_site;
int ugp_genotypes_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_genotype_select(ugp_mat *mat, const uint32_t *nodes /* BFS; NULL: all leaves */, uint64_t n, uint32_t *n_cols, uint64_t *n_sites);
int ugp_genotype_columns(ugp_mat *mat, uint32_t *nodes /* [n_cols] BFS, depth-first order */);
int ugp_genotype_sites(ugp_mat *mat, uint64_t lo, uint64_t hi, ugp_gt_site *out /* [hi - lo] */);
int ugp_genotype_rows(ugp_mat *mat, uint64_t lo, uint64_t hi, uint8_t *codes /* [(hi - lo) * n_cols] */);
int ugp_genotype_rows_chunked(ugp_mat *mat, uint64_t lo, uint64_t hi, uint8_t *codes, uint64_t chunk_cells);
/* Bench hook: milliseconds of device time of the row kernel alone over sites [lo, hi), without the copy to the host; mean of `reps` runs. */
int ugp_genotype_rows_time(ugp_mat *mat, uint64_t lo, uint64_t hi, uint32_t reps, double *ms);
/* matUtils summary (matUtils/summary.cpp): the mutation table (-m, :139-174), the RoHo records (-R without -E, :343-506) and the
 * clade counts (-c :88-137, -C :297-341).  ugp_summary_attach shares the depth-first tables of `tree` exactly as
 * ugp_genotypes_attach does (the handle's tree; arrays are copied; mut_par is needed; mut_nuc / mut_par of non-masked mutations in
 * 1 .. 15, UGP_ERR_UNSUPPORTED otherwise; tables built from other mutation arrays: UGP_ERR_INVALID) and builds, once per handle, the
 * OCCURRENCE LIST -- every mutation entry sorted by (key, depth-first position of its node) -- and the strict-descendant leaf
 * count of every node.  The KEY of an entry is what Mutation::get_string() prints: (position, mut_par as stored, mut_nuc); every
 * masked entry (mut_pos < 0) has the one key "MASKED".
 * ugp_summary_mutations: the distinct non-masked keys with the number of entries that carry them, over all nodes, root included,
 *   ascending by (pos, par, nuc).  out[0 .. min(cap, *n_out)) is written and *n_out is the true count.
 * ugp_summary_roho: one record per (parent n, key) that write_roho_table reports, ascending by the depth-first position of n (records
 *   of one parent in depth-first order of their entry; the host orders them by name).  The candidates of n are the keys on its
 *   NON-LEAF children (masked counts as a key; a key stored twice on one child is one candidate; when two non-leaf children carry a
 *   key the LATER one owns it and the earlier is not reported; the root's own entries are no candidates).  A candidate is erased
 *   when its key occurs on a node of n's subtree at depth >= depth(n) + 2 -- under the owning child or under a sibling; a leaf CHILD
 *   of n with the key does not erase it.  With lc(c) the leaves strictly below c: a record needs lc(owner) > 5 and at least one OTHER
 *   non-leaf child with lc > 5; offspring_with = lc(owner); median_without = the middle of the sorted lc > 5 of those others, for
 *   an even number (a + b) / 2 in integer division (:461-465); child_count = the non-leaf children of n (ccheck.size()).  `entry` is
 *   the index in tree->mut_off's CSR of the first entry with the key on `child`.  cap / *n_out as above.
 * The _chunked twins (test hooks) set the work-items per launch window (0: default): list entries for the mutation table, candidate
 *   entries (those of non-leaf nodes other than the root) for RoHo.
 * ugp_summary_clades: per annotation column c the nodes col_off[c] .. col_off[c + 1] of `nodes` (BFS; a node twice in one column is
 *   UGP_ERR_INVALID) carry a non-empty annotation.  Per listed node: incl = the leaves strictly below it, excl = the leaves whose
 *   nearest listed STRICT ancestor in that column it is (a listed leaf counts nothing).  leaf_clade[c * n_leaves + i] = that
 *   ancestor (BFS) for the i-th leaf in BFS order (Tree::get_leaves), or UINT32_MAX. */
typedef struct ugp_sm_mutation {
    int32_t pos;
    uint8_t par, nuc;    /* 4-bit codes                                            */
    uint8_t pad[2];
    uint32_t count;      /* entries with this key                                  */
} ugp_sm_mutation;
typedef struct ugp_sm_roho {
    uint32_t parent, child;      /* BFS indices                                    */
    uint32_t entry;              /* index into the caller's mutation CSR           */
    uint32_t child_count;        /* non-leaf children of parent                    */
    uint32_t offspring_with;     /* leaves strictly below child                    */
    uint32_t median_without;     /* med_non before it becomes a float              */
} ugp_sm_roho;
int ugp_summary_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_summary_mutations(ugp_mat *mat, ugp_sm_mutation *out, uint64_t cap, uint64_t *n_out);
int ugp_summary_mutations_chunked(ugp_mat *mat, ugp_sm_mutation *out, uint64_t cap, uint64_t *n_out, uint64_t chunk_items);
int ugp_summary_roho(ugp_mat *mat, ugp_sm_roho *out, uint64_t cap, uint64_t *n_out);
int ugp_summary_roho_chunked(ugp_mat *mat, ugp_sm_roho *out, uint64_t cap, uint64_t *n_out, uint64_t chunk_items);
int ugp_summary_clades(ugp_mat *mat, const uint64_t *col_off /* [n_cols + 1] */, const uint32_t *nodes /* BFS */, uint64_t n_cols,
                       uint32_t *incl /* [col_off[n_cols]] */, uint32_t *excl /* [col_off[n_cols]] */, uint32_t *leaf_clade /* [n_cols * n_leaves] */);
/* Bench hook: milliseconds of device time of the occurrence-list sort alone and of the RoHo kernel alone over every candidate
 * (no compaction, no copy to the host); mean of `reps` runs. */
int ugp_summary_time(ugp_mat *mat, uint32_t reps, double *sort_ms, double *roho_ms);
/* matUtils summary --translate (matUtils/translate.cpp: translate_main, do_mutations in TSV mode): per node the codons its mutations
 * touch, with their letters before and after.  ugp_translate_attach shares the depth-first tables of `tree` exactly as
 * ugp_genotypes_attach does (the handle's tree; arrays are copied; mut_par is needed; mut_nuc / mut_par of non-masked mutations in
 * 1 .. 15, UGP_ERR_UNSUPPORTED otherwise; tables built from other mutation arrays: UGP_ERR_INVALID).
 * ugp_translate_codons: the codon table in the reference's creation order (build_codon_map); codon c has the slots
 *   slot_pos[3c .. 3c + 2] (1-based genome positions as mut_pos; a '+' codon ascends, a '-' codon descends) with the letters
 *   slot_init[3c .. 3c + 2] they hold before any mutation ('-': the complemented FASTA).  The codons of a position rank by their
 *   index.  A slot position < 1 or >= 2^28, or two equal ones within a codon, are UGP_ERR_INVALID.  The table replaces any earlier
 *   one; n_codons = 0 is a table without codons.
 * A position is CODING when a slot holds it.  The OWNER of a position on a node is the node's first non-masked entry there; the
 *   STATE BEFORE node v at a slot with position p is the letter of mut_nuc of the owner of p on the nearest strict ancestor of v
 *   that has one, else the slot's initial letter.  An owner at a coding position is INCONSISTENT when the letter of its mut_par as
 *   stored differs from the state before its node at a slot that holds its position (the reference's walk is then history
 *   dependent: undoing a node does not restore what was there).  A node with two non-masked entries at one coding position is a
 *   DUPLICATE node.  Masked entries (mut_pos < 0) are skipped; a repeated non-coding position is nobody's business.
 * ugp_translate: one record per (node, codon with an owner of the node in one of its slots), ascending by (depth-first position of
 *   the node, lowest such position of the codon on that node, codon index) -- the order do_mutations first touches them.
 *   before[s] = the state before the node at slot s, after[s] = the letter of mut_nuc of the node's owner at slot s, else
 *   before[s]; ent[s] = that owner's index in tree->mut_off's CSR, else UINT32_MAX.  Letters are those of get_nuc
 *   ("NACMGRSVTWYHKDBN").  out[0 .. min(cap, *n_out)) is written and *n_out is the true count.  `info` (may be NULL) is filled by
 *   every call that ran; first_inconsistent is the first such entry in depth-first order of its node, then stored order (CSR index),
 *   first_duplicate the first such node in depth-first order (BFS index), UINT32_MAX when there is none.  When n_inconsistent or
 *   n_duplicate is non-zero the call returns UGP_ERR_UNSUPPORTED, *n_out = 0 and nothing is written to `out`: the caller walks
 *   the tree serially instead.  A call before the attach or before the codon table is UGP_ERR_INVALID and names the missing call.
 * ugp_translate_chunked (test hook) sets the work-items -- (owner at a coding position, codon of that position) pairs -- per launch
 *   window (0: default). */
typedef struct ugp_tr_record {
    uint32_t node;               /* BFS index                                      */
    uint32_t codon;              /* index into the codon table                     */
    uint8_t before[3], after[3]; /* letters per slot                               */
    uint8_t pad[2];
    uint32_t ent[3];             /* the node's entry at each slot, or UINT32_MAX   */
} ugp_tr_record;
typedef struct ugp_tr_info {
    uint64_t n_records;          /* as counted, also when the call refuses         */
    uint64_t n_nodes;            /* nodes with at least one record                 */
    uint64_t n_inconsistent, n_duplicate;
    uint32_t first_inconsistent; /* CSR index of the entry                         */
    uint32_t first_duplicate;    /* BFS index of the node                          */
} ugp_tr_info;
int ugp_translate_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_translate_codons(ugp_mat *mat, uint64_t n_codons, const int32_t *slot_pos /* [3 n_codons] */, const uint8_t *slot_init /* [3 n_codons] */);
int ugp_translate(ugp_mat *mat, ugp_tr_record *out, uint64_t cap, uint64_t *n_out, ugp_tr_info *info);
int ugp_translate_chunked(ugp_mat *mat, ugp_tr_record *out, uint64_t cap, uint64_t *n_out, ugp_tr_info *info, uint64_t chunk_items);
/* Bench hook: milliseconds of device time of the passes of ugp_translate alone (records, scan, compaction over every window; no copy to
 * the host); mean of `reps` runs. */
int ugp_translate_time(ugp_mat *mat, uint32_t reps, double *ms);
/* matUtils extract --closest-relatives / --within-distance (get_closest_samples, matUtils/select.cpp:577-714) for a batch of samples.
 * ugp_relatives_attach shares the depth-first tables of `tree` (the handle's tree; arrays are copied; tables built from other mutation
 * arrays: UGP_ERR_INVALID, nothing changed) and builds, once per handle, the leaves in depth-first order with a range minimum over
 * their cum (blocks of UGP_REL_BLOCK leaves), the leaves ordered by (cum, depth-first rank) and, when name_rank is given, a range
 * minimum over the name ranks in that order.  name_rank [n] by BFS index is a permutation of 0 .. n - 1: the order of the
 * identifiers under std::string::operator< (unsigned bytes); NULL: no ranks.  A second attach replaces the first.
 * With cum[v] the mutation entries on the root path of v (v and masked entries included), nm[v] those on v itself, t the sample,
 * p_0 = parent(t), p_1, ... its ancestors, c_0 = t and c_j = p_{j-1}: the RING of level j is the leaves of subtree(p_j) outside
 * subtree(c_j); a ring leaf l is d(l) = cum[t] + cum[l] - 2 cum[p_j] away; the level bound is L_j = cum[p_0] - cum[p_j] + nm[p_j].
 * ugp_relatives_closest (fixed_k = false): levels 0, 1, ... in order; m_j = the smallest d of the ring (an empty ring has none); a
 *   strictly smaller m_j replaces the list, an equal one appends; the climb stops after the first level with m_j < L_j, or after
 *   the root's.  The list is, level by level, the ring leaves at the final distance in depth-first order.
 * ugp_relatives_within (fixed_k = true): the ring leaves with d <= threshold, level by level, each level in depth-first order; the
 *   climb stops after the first level with L_j > threshold, or after the root's.
 * Two quirks of the reference are kept: L_j leaves out nm[t], and dist is 0 when there are no relatives.  The root has none.
 * Sample i is a node (BFS index; any node).  info[i]: count = the length of its list, levels = the levels processed, dist = the
 * final distance (closest mode; 0 in within mode), best = the BFS index of the relative with the smallest name rank among the
 * closest (UINT32_MAX without relatives, without ranks, and in within mode).  out_off NULL: no lists (out_nodes and cap are
 * ignored).  Else list i is out_nodes[out_off[i] .. out_off[i + 1]) (BFS indices); out_off [n + 1] is always complete,
 * out_nodes[0 .. min(cap, *n_out)) is written and *n_out is the true total in either case.  An out-of-range node or a call before
 * the attach is UGP_ERR_INVALID before anything is written.  Samples run in chunks of bounded device workspace; the _chunked
 * twins (test hooks) set the samples per chunk (0: default) and with them the list entries per window (16 per sample). */
#define UGP_REL_BLOCK 16
typedef struct ugp_rel_info { uint32_t dist, count, levels, best; } ugp_rel_info;
int ugp_relatives_attach(ugp_mat *mat, const ugp_tree_desc *tree, const uint32_t *name_rank /* [n] by BFS index, or NULL */);
int ugp_relatives_closest(ugp_mat *mat, uint64_t n, const uint32_t *nodes /* BFS, any node */, ugp_rel_info *info /* [n] */,
                          uint64_t *out_off /* [n + 1], or NULL: no lists */, uint32_t *out_nodes, uint64_t cap, uint64_t *n_out);
int ugp_relatives_within(ugp_mat *mat, uint64_t n, const uint32_t *nodes, uint32_t threshold, ugp_rel_info *info,
                         uint64_t *out_off, uint32_t *out_nodes, uint64_t cap, uint64_t *n_out);
int ugp_relatives_closest_chunked(ugp_mat *mat, uint64_t n, const uint32_t *nodes, ugp_rel_info *info, uint64_t *out_off,
                                  uint32_t *out_nodes, uint64_t cap, uint64_t *n_out, uint32_t chunk_samples);
int ugp_relatives_within_chunked(ugp_mat *mat, uint64_t n, const uint32_t *nodes, uint32_t threshold, ugp_rel_info *info,
                                 uint64_t *out_off, uint32_t *out_nodes, uint64_t cap, uint64_t *n_out, uint32_t chunk_samples);
/* Bench hook: milliseconds of device time of the kernels alone over these samples -- count_ms the climb with its counts and the prefix
 * sum, fill_ms the second climb that writes the lists (they stay on the device) -- mean of `reps` runs after one warm-up run.
 * within = 0: closest mode (threshold ignored). */
int ugp_relatives_time(ugp_mat *mat, uint64_t n, const uint32_t *nodes, int within, uint32_t threshold, uint32_t reps, double *count_ms,
                       double *fill_ms);
/* matUtils extract's sample selectors (matUtils/select.cpp: get_mutation_samples :67-111, get_leaves_ids under get_clade_samples and
 * -I, get_mrca_samples :570-575) as bitmaps over LEAF RANKS: leaf r is the r-th leaf of the depth-first expansion, bit r & 63 of
 * word r >> 6; a bitmap has (n_leaves + 63) / 64 words and the bits past the last leaf are zero in every bitmap written here.
 * ugp_select_attach shares the depth-first tables of `tree` (the handle's tree; arrays are copied; tables built from other mutation
 * arrays: UGP_ERR_INVALID, nothing changed) and builds, once per handle, the leaves in depth-first order and per node the half-open
 * range of leaf ranks below it.  A second attach replaces the first.  A call before the attach is UGP_ERR_INVALID.
 * ugp_select_leaves: bfs_by_rank[r] = the BFS index of leaf r (NULL: not written); *n_leaves = their number (NULL: not written).
 * ugp_select_mutations: leaf l is selected by query q = (pos, nuc) exactly when the nearest node on l's root path, l included, with
 *   a non-masked entry at pos has mut_nuc == nuc in the FIRST such entry it stores (equality of the stored code, no bit test).  A
 *   leaf with no such node is not selected whatever nuc is: a query for the reference base selects only leaves under a
 *   back-mutation (get_mutation_samples read literally).  pos < 0 and positions above every entry select nobody.  words = the OR
 *   over all queries, counts[q] = the leaves of query q alone.
 * ugp_select_subtrees: words = the union of the leaves below the given nodes (a leaf node selects itself), counts[i] = the leaves
 *   below node i alone.  A node out of range is UGP_ERR_INVALID before anything is written.
 * ugp_select_mrca: *node = the deepest node whose subtree holds every leaf set in `words` (bits past the last leaf are ignored),
 *   *n_below = the leaves below it.  An empty bitmap is UGP_ERR_INVALID.
 * The _chunked twins (test hooks) set the queries, or the disjoint rank ranges, staged per launch (0: default). */
int ugp_select_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_select_leaves(ugp_mat *mat, uint32_t *bfs_by_rank /* [n_leaves], or NULL */, uint64_t *n_leaves /* or NULL */);
int ugp_select_mutations(ugp_mat *mat, uint64_t n_mut, const int32_t *pos, const uint8_t *nuc, uint64_t *words, uint64_t *counts /* [n_mut] */);
int ugp_select_mutations_chunked(ugp_mat *mat, uint64_t n_mut, const int32_t *pos, const uint8_t *nuc, uint64_t *words, uint64_t *counts,
                                 uint32_t chunk_queries);
int ugp_select_subtrees(ugp_mat *mat, uint64_t n, const uint32_t *nodes /* BFS, any node */, uint64_t *words, uint64_t *counts /* [n] */);
int ugp_select_subtrees_chunked(ugp_mat *mat, uint64_t n, const uint32_t *nodes, uint64_t *words, uint64_t *counts, uint32_t chunk_ranges);
int ugp_select_mrca(ugp_mat *mat, const uint64_t *words, uint32_t *node /* BFS */, uint64_t *n_below);
/* Bench hook: milliseconds of device time of the mutation kernel alone over these queries (the bitmap and the counts stay on the
 * device); mean of `reps` runs after one warm-up run. */
int ugp_select_time(ugp_mat *mat, uint64_t n_mut, const int32_t *pos, const uint8_t *nuc, uint32_t reps, double *ms);
/* node_excess_mutations and node_imputed_mutations of mapper2_body (usher_mapper.cpp:167-504 with compute_vecs, as pass 2 of
 * usher_common.cpp:426-449 runs it on the placement node) for (sample, node) pairs: with ugp_place_batch the whole of
 * usher_common.cpp:342-449.  ugp_vectors_attach shares the depth-first tables of `tree` (the handle's tree; arrays are copied,
 * mut_par included: it is what the entries of part 1 report; tables built from other mutation arrays: UGP_ERR_INVALID, nothing
 * changed; an allele above 15: UGP_ERR_UNSUPPORTED).  A second attach replaces the first.  A call before the attach is
 * UGP_ERR_INVALID.
 * Pair i is (sample[i] -- an index into q; NULL: i --, node[i] -- BFS).  Every entry is (pos, ref, par, nuc) = (position, ref_nuc,
 * par_nuc, mut_nuc).  The excess list of a pair is, in this order,
 *   1. the node's own entries that the branch loop (:190-264) keeps, in stored order, par as stored: info.n_branch of them;
 *   2. one entry per non-missing row of the sample that the ancestral state g(p) does not explain (:292-388), in row order:
 *      par = g(p), the allele of the nearest node on the root path with a non-masked entry at p (the node's own entry only when
 *      part 1 kept it; the root's own for the root; none: the row's ref), nuc = the row's ref when the row holds it, else its
 *      lowest set bit, and nuc != par (for rows that pass the row checks -- a one-hot ref, a non-zero mask -- a row that g(p) does
 *      not explain always has nuc != par: nuc is a bit of the row or its ref, and g(p) shares no bit with the row);
 *   3. one entry (g(p) -> ref) per position with an ancestral state other than its reference and no row in the sample (:393-445),
 *      in ascending position.  For the root, its masked entries with nuc != ref give one each as well: they come first, in stored
 *      order (the reference's unstable sort leaves their mutual order open).
 * The imputed list holds one entry per ambiguous row (more than one bit), in row order (:322-335, :341-351, :375-377).
 * info: n_excess, n_imputed, n_branch; set_difference = the entries of parts 2 and 3 (the reference's figure for an eligible node,
 * one less than it for any other); has_unique = the branch loop's; eligible = the predicate of :454-455.  A pair whose node stores
 * one non-masked position twice has refused = 1, every other field 0 and both lists empty: the reference's answer depends on an
 * unstable sort there, and the caller runs such a pair on the host.
 * Rows are checked as ugp_place_batch checks them (same errors).  A sample index >= q->n_queries or a node >= n_nodes is
 * UGP_ERR_INVALID before anything is written.  ex_off / im_off [n_pairs + 1] are always complete, excess[0 .. min(ex_cap,
 * *n_excess)) is written and *n_excess is the true total; the same for imputed.  Pairs come in any order and may repeat.  The
 * _chunked twin (test hook) sets the pairs per launch window (0: default). */
typedef struct ugp_vec_entry { int32_t pos; uint8_t ref, par, nuc, pad; } ugp_vec_entry;
typedef struct ugp_vec_info {
    uint32_t n_excess, n_imputed;
    uint32_t n_branch;        /* leading excess entries that come from the node's own branch (loop 1) */
    int32_t  set_difference;  /* excess entries of loops 2 and 3: the score before the "+1" of an ineligible node */
    uint8_t  has_unique, eligible, refused, pad;
} ugp_vec_info;
int ugp_vectors_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_vectors(ugp_mat *mat, const ugp_queries *q, uint64_t n_pairs, const uint32_t *sample, const uint32_t *node, ugp_vec_info *info,
                uint64_t *ex_off, ugp_vec_entry *excess, uint64_t ex_cap, uint64_t *n_excess,
                uint64_t *im_off, ugp_vec_entry *imputed, uint64_t im_cap, uint64_t *n_imputed);
int ugp_vectors_chunked(ugp_mat *mat, const ugp_queries *q, uint64_t n_pairs, const uint32_t *sample, const uint32_t *node, ugp_vec_info *info,
                        uint64_t *ex_off, ugp_vec_entry *excess, uint64_t ex_cap, uint64_t *n_excess,
                        uint64_t *im_off, ugp_vec_entry *imputed, uint64_t im_cap, uint64_t *n_imputed, uint32_t chunk_pairs);
/* Bench hook: milliseconds of device time of the kernels alone over these pairs -- count_ms the counting pass with its prefix sums,
 * fill_ms the pass that writes the lists and orders part 3 (they stay on the device) -- mean of `reps` runs after one warm-up run. */
int ugp_vectors_time(ugp_mat *mat, const ugp_queries *q, uint64_t n_pairs, const uint32_t *sample, const uint32_t *node, uint32_t reps,
                     double *count_ms, double *fill_ms);
/* matUtils mask (matUtils/mask.cpp: restrictSamples :802-905, restrictMutationsLocally :703-800), both in closed form over the
 * depth-first ranges.  A mutation's KEY is (position, parent allele as stored, allele); entries are those of the mutation CSR.
 * ugp_mask_attach shares the depth-first tables of `tree` (the handle's tree; arrays are copied; tables built from other mutation
 * arrays: UGP_ERR_INVALID, nothing changed; an allele above 15: UGP_ERR_UNSUPPORTED) and builds, once per handle, the leaf-rank
 * ranges and per entry its stored alleles.  A second attach replaces the first.  A call before the attach is UGP_ERR_INVALID.
 * ugp_mask_restricted: the n named nodes (BFS; one given twice counts once; n = 0 and a node out of range are UGP_ERR_INVALID before
 *   anything is written) must be leaves: a named internal node is UGP_ERR_UNSUPPORTED (roots can nest then; the caller walks), and so
 *   is a tree whose positions reach past the bounded key table.  With full(v): every leaf below v is named, and F: the inner nodes
 *   that are full and have a leaf child, the restricted roots are the nodes of F with no proper ancestor in F and the named leaves
 *   whose parent is not full (or absent).  roots_bfs = the first min(roots_cap, *n_roots) of them in depth-first order.
 *   entry_masked[e] = 1 exactly when entry e is non-masked, lies at or below a root, and no non-masked entry with the same key lies
 *   on a node below no root; else 0.  *n_masked = their number.  The tree arrays are not changed.
 * ugp_mask_mutations: line l = (pos, par, nuc, node_bfs, excluded nodes excl_bfs[excl_off[l] .. excl_off[l + 1])); par and nuc are
 *   4-bit codes, 15 matches any.  Line l matches a non-masked entry on node v when the position is equal, par and nuc match the
 *   stored parent allele and allele, v lies at or below the line's node, and v lies at or below no excluded node that is a strict
 *   descendant of the line's node (other excluded nodes, and indices that are no node, have no effect).  first_line[e] = the first
 *   line in the order given that matches entry e, or UINT32_MAX; entries with skip[e] != 0 (skip may be NULL) never match.
 *   counts[l] = the entries with first_line == l.  A line's node out of range, an allele above 15 or offsets that do not ascend
 *   from 0 are UGP_ERR_INVALID before anything is written.  The _chunked twin (test hook) sets the lines staged per launch
 *   (0: default). */
int ugp_mask_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_mask_restricted(ugp_mat *mat, uint64_t n, const uint32_t *leaves_bfs, uint8_t *entry_masked /* [n_muts] */,
                        uint32_t *roots_bfs /* [roots_cap] */, uint64_t roots_cap, uint64_t *n_roots, uint64_t *n_masked);
int ugp_mask_mutations(ugp_mat *mat, uint64_t n_lines, const int32_t *pos, const uint8_t *par, const uint8_t *nuc, const uint32_t *node_bfs,
                       const uint64_t *excl_off /* [n_lines + 1] */, const uint32_t *excl_bfs, const uint8_t *skip /* [n_muts], or NULL */,
                       uint32_t *first_line /* [n_muts] */, uint64_t *counts /* [n_lines] */);
int ugp_mask_mutations_chunked(ugp_mat *mat, uint64_t n_lines, const int32_t *pos, const uint8_t *par, const uint8_t *nuc,
                               const uint32_t *node_bfs, const uint64_t *excl_off, const uint32_t *excl_bfs, const uint8_t *skip,
                               uint32_t *first_line, uint64_t *counts, uint32_t chunk_lines);
/* Bench hook: milliseconds of device time of the passes alone, no copies: *restricted_ms for the n named leaves (n = 0: not run, 0),
 * *mutations_ms for the lines (n_lines = 0: not run, 0; no more than one default batch); each the mean of `reps` runs after one
 * warm-up run. */
int ugp_mask_time(ugp_mat *mat, uint64_t n, const uint32_t *leaves_bfs, uint64_t n_lines, const int32_t *pos, const uint8_t *par,
                  const uint8_t *nuc, const uint32_t *node_bfs, const uint64_t *excl_off, const uint32_t *excl_bfs, uint32_t reps,
                  double *restricted_ms, double *mutations_ms);
/* The subtree induced by a selection (mutation_annotated_tree.cpp: get_subtree :1577-1685 with Node::add_mutation :720-752), in
 * closed form over the depth-first ranges; no pair of samples is visited and nothing climbs.  S is the set of the n named nodes (BFS;
 * leaf or internal; one given twice counts once).  The KEPT nodes are S and every lowest common ancestor of two members of S: v is
 * kept exactly when it is in S or at least two of its children have a member of S at or below them.  Kept nodes come in the
 * depth-first order of the tree.  The SUBTREE PARENT of a kept node is its nearest proper ancestor that is kept; the first kept node
 * is the subtree's root and has none.  The CHAIN of a kept node v with subtree parent u is the path from u (exclusive) down to v
 * (inclusive); the root's chain starts at the tree's root (inclusive).  Every node with a member of S at or below it lies in exactly
 * one chain, whose kept node is its OWNER; every other node has none.
 * The MERGED ENTRIES of v are what add_mutation leaves of the entries of chain(v), taken top-down and in stored order within a node.
 * Per position the state is empty or one entry; for each entry e at that position: state empty -- the state becomes a copy of e
 * (nothing is checked, also when e.par == e.nuc); state s with s.par != e.nuc -- s.nuc = e.nuc; s.par == e.nuc and s.nuc == e.par --
 * the state becomes empty (a later entry opens a new one with its own ref and par); s.par == e.nuc and s.nuc != e.par -- a
 * DISAGREEMENT: e is skipped, the state stays, and the call counts it (get_subtree ignores add_mutation's false).  Masked entries
 * take part with their stored position (-1) and stored alleles.  The result ascends by position.  A merged entry is returned as
 * its position, the index in the caller's CSR of the entry that OPENED its state (the caller copies ref, par and every other field
 * from that entry) and its final allele.
 * ugp_subtree_attach shares the depth-first tables of `tree` (the handle's tree; arrays are copied; tables built from other mutation
 * arrays: UGP_ERR_INVALID, nothing changed; an allele above 15: UGP_ERR_UNSUPPORTED) and keeps per entry its stored alleles.  A second
 * attach replaces the first.  A call before the attach is UGP_ERR_INVALID and names the missing call.
 * ugp_subtree_nodes: n = 0 or a node out of range is UGP_ERR_INVALID before anything is written.  kept_bfs[k] = kept node k (BFS),
 *   kept_parent[k] = the index in the kept list of its subtree parent (UINT32_MAX: the root), ent_off[k] = the index of its first
 *   merged entry (its last one is in front of ent_off[k + 1], or of *n_entries for the last kept node).  [0 .. min(cap, *n_kept)) of
 *   the three is written; *n_kept and *n_entries are always the true counts.  `info` (may be NULL): the distinct selected nodes, the
 *   tree entries on the chains, the disagreements, the first kept node in depth-first order with one (BFS; UINT32_MAX: none) and
 *   the nodes of the longest chain.
 * ugp_subtree_entries: the merged entries of the last ugp_subtree_nodes call, kept node after kept node; [0 .. min(cap, *n_out)) is
 *   written, *n_out is the true count.  ugp_subtree_owner: owner[i] = the index in the kept list of the owner of node i (BFS; any
 *   node; out of range or n = 0: UGP_ERR_INVALID), or UINT32_MAX, for the last ugp_subtree_nodes call.  Either before any such call
 *   is UGP_ERR_INVALID.
 * The gather of the chains' entries and the merge run in launch windows; the _chunked twin (test hook) sets the items per window
 * (0: default). */
typedef struct ugp_subtree_info {
    uint64_t n_selected;         /* distinct selected nodes                         */
    uint64_t n_gathered;         /* tree entries on the chains                      */
    uint64_t n_disagree;         /* entries add_mutation refuses                    */
    uint64_t longest_chain;      /* nodes of the longest chain                      */
    uint32_t first_disagree;     /* BFS index, UINT32_MAX: none                     */
    uint32_t pad;
} ugp_subtree_info;
int ugp_subtree_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_subtree_nodes(ugp_mat *mat, uint64_t n, const uint32_t *nodes_bfs, uint32_t *kept_bfs /* [cap] */, uint32_t *kept_parent /* [cap] */,
                      uint64_t *ent_off /* [cap] */, uint64_t cap, uint64_t *n_kept, uint64_t *n_entries, ugp_subtree_info *info /* or NULL */);
int ugp_subtree_nodes_chunked(ugp_mat *mat, uint64_t n, const uint32_t *nodes_bfs, uint32_t *kept_bfs, uint32_t *kept_parent, uint64_t *ent_off,
                              uint64_t cap, uint64_t *n_kept, uint64_t *n_entries, ugp_subtree_info *info, uint64_t chunk_items);
int ugp_subtree_entries(ugp_mat *mat, int32_t *pos /* [cap] */, uint32_t *first_entry /* [cap] */, uint8_t *nuc /* [cap] */, uint64_t cap,
                        uint64_t *n_out);
int ugp_subtree_owner(ugp_mat *mat, uint64_t n, const uint32_t *nodes_bfs, uint32_t *owner /* [n] */);
/* Bench hook: milliseconds of device time of the passes alone, no copies, for the n named nodes: *nodes_ms the marks, the scans and
 * the kept list, *merge_ms the gather, the sort, the merge and the compaction; each the mean of `reps` runs after one warm-up run. */
int ugp_subtree_time(ugp_mat *mat, uint64_t n, const uint32_t *nodes_bfs, uint32_t reps, double *nodes_ms, double *merge_ms);
/* Many induced subtrees of the attached tree in one call (matUtils/convert.cpp: get_minimum_subtrees :665-798 builds one per
 * neighbourhood).  Selection b is nodes_bfs[sel_off[b] .. sel_off[b + 1]); its result is exactly what ugp_subtree_nodes and
 * ugp_subtree_entries return for that selection alone, by the definitions above.  The device work and workspace of a selection
 * follow its WINDOW -- the depth-first range of its lowest common ancestor, the entries on those nodes and the entries on the
 * ancestor's root path -- not the tree: selections are laid end to end in GROUPS of at most group_positions window positions
 * (0: the default, half the tree's nodes and half its entries, so that a group needs no more memory than the single call's
 * tables; a selection whose window alone is larger runs as a group of its own), and the passes run once per group.
 * ugp_subtree_batch: n_sel = 0, an empty selection, a node out of range or descending sel_off is UGP_ERR_INVALID before anything is
 *   written.  kept_off[b] / entry_off[b] ([n_sel + 1]) = the first kept node / merged entry of selection b in the batch's lists;
 *   info[b] (info may be NULL): the single call's counts for selection b, its kept nodes and merged entries, and its lowest common
 *   ancestor (BFS), which is its first kept node.
 * ugp_subtree_batch_nodes: the kept nodes of the last batch, selection after selection, each slice in depth-first order.
 *   kept_parent[k] is an index WITHIN the slice of k's selection (UINT32_MAX: the slice's root, whose chain starts at the tree's
 *   root); ent_off[k] indexes the batch's entry list (the last entry of k is in front of ent_off[k + 1], or of the entry count for
 *   the last kept node).  ugp_subtree_batch_entries: the merged entries of the last batch.  Both follow the single call's cap
 *   convention: [0 .. min(cap, *n_out)) is written, *n_out is the true count; either before any batch is UGP_ERR_INVALID.
 * The batch keeps its own result: ugp_subtree_entries and ugp_subtree_owner go on answering for the last ugp_subtree_nodes call, and
 * a single call leaves the last batch's lists as they are.  The _chunked twin (test hook) sets the group budget and the items
 * per launch window of the gather and the merge (0: default). */
typedef struct ugp_subtree_batch_info {
    uint64_t n_selected;         /* distinct selected nodes                         */
    uint64_t n_kept;             /* kept nodes                                      */
    uint64_t n_entries;          /* merged entries                                  */
    uint64_t n_gathered;         /* tree entries on the chains                      */
    uint64_t n_disagree;         /* entries add_mutation refuses                    */
    uint64_t longest_chain;      /* nodes of the longest chain                      */
    uint32_t first_disagree;     /* BFS index, UINT32_MAX: none                     */
    uint32_t lca;                /* BFS index of the lowest common ancestor         */
} ugp_subtree_batch_info;
int ugp_subtree_batch(ugp_mat *mat, uint64_t n_sel, const uint64_t *sel_off /* [n_sel + 1] */, const uint32_t *nodes_bfs,
                      uint64_t *kept_off /* [n_sel + 1] */, uint64_t *entry_off /* [n_sel + 1] */, ugp_subtree_batch_info *info /* [n_sel] or NULL */);
int ugp_subtree_batch_chunked(ugp_mat *mat, uint64_t n_sel, const uint64_t *sel_off, const uint32_t *nodes_bfs, uint64_t *kept_off,
                              uint64_t *entry_off, ugp_subtree_batch_info *info, uint64_t group_positions, uint64_t chunk_items);
int ugp_subtree_batch_nodes(ugp_mat *mat, uint32_t *kept_bfs /* [cap] */, uint32_t *kept_parent /* [cap] */, uint64_t *ent_off /* [cap] */,
                            uint64_t cap, uint64_t *n_out);
int ugp_subtree_batch_entries(ugp_mat *mat, int32_t *pos /* [cap] */, uint32_t *first_entry /* [cap] */, uint8_t *nuc /* [cap] */, uint64_t cap,
                              uint64_t *n_out);
/* Bench hook: as ugp_subtree_time, for the passes of every group of the batch (default budget), summed over the groups. */
int ugp_subtree_batch_time(ugp_mat *mat, uint64_t n_sel, const uint64_t *sel_off, const uint32_t *nodes_bfs, uint32_t reps, double *nodes_ms,
                           double *merge_ms);
/* matUtils summary --haplotype (matUtils/summary.cpp: count_haplotypes :182-218, write_haplotype_table :244-264): the distinct
 * HAPLOTYPES of the leaves with the number of leaves that carry each.  The reference walks the nodes in depth-first order with a
 * std::map<int,int8_t> per node: a node starts from its parent's map (the root from an empty one) and applies its entries in stored
 * order -- an entry with mut_nuc == its own stored ref_nuc erases the position, any other sets map[position] = mut_nuc; mut_par
 * plays no part.  Masked entries (mut_pos < 0) are skipped: they erase a negative position that nothing sets.  So the STATE of a
 * position at a node is that of the last non-masked entry at it on the deepest node of the root path (the node included) that has
 * one; it is OFF THE REFERENCE when that entry's mut_nuc differs from that entry's ref_nuc, and the haplotype of a node is the set
 * of (position, mut_nuc) of the positions off the reference.  Every leaf counts for its haplotype (a tree that is only a root counts
 * the root); internal nodes are never counted.
 * ugp_haplotypes_attach shares the depth-first tables of `tree` exactly as ugp_summary_attach does (the handle's tree; arrays are
 * copied; mut_par is not read; tables built from other mutation arrays: UGP_ERR_INVALID, nothing changed) and builds, once per
 * handle, the leaves in depth-first order.  A second attach replaces the first.  A call before the attach is UGP_ERR_INVALID and
 * names the missing call.  A node with two non-masked entries at one position is a DUPLICATE node (the walk takes its last entry,
 * the tables' owner is its first): with any, ugp_haplotype_groups and ugp_haplotype_sets return UGP_ERR_UNSUPPORTED, *n_out = 0 and
 * nothing is written; the caller walks the tree serially instead.
 * ugp_haplotype_groups: one record per distinct haplotype: leaf = the BFS index of its first leaf in depth-first order, count = its
 *   leaves, size = its (position, allele) pairs; records ascend by the depth-first position of `leaf`.  out[0 .. min(cap, *n_out))
 *   is written and *n_out is the true count.  The groups are the runs of a sort of the leaves by a 128-bit FINGERPRINT of their
 *   haplotype (a sum, modulo 2^64 in each of two lanes, of a fixed mix of every pair of the set), and every leaf that is not the
 *   first of its run is then compared exactly with the leaf in front of it: every position with an entry on either leaf's path
 *   below their lowest common ancestor must have the same state for both, and the sizes must agree.  A leaf that differs is a
 *   COLLISION: with any the call returns UGP_ERR_UNSUPPORTED, *n_out = 0 and nothing is written -- no table is returned that has
 *   not been verified.  `info` (may be NULL) is filled by every call that ran, also when it refuses; first_duplicate is the first
 *   duplicate node in depth-first order (BFS index), UINT32_MAX when there is none; n_visited the entries the comparison read.
 * ugp_haplotype_groups_hashed (test hook): only the low hash_bits (0 .. 128; more is UGP_ERR_INVALID) of the fingerprint take part
 *   in the sort and in the runs; 128 is the plain call, 0 puts every leaf into one run.
 * ugp_haplotype_sets: the haplotypes of the n given leaves (BFS; an index out of range or an internal node is UGP_ERR_INVALID before
 *   anything is written) as a CSR: off[n + 1] is always complete, set i is pos / nuc[off[i] .. off[i + 1]), ascending by position,
 *   nuc the stored 4-bit code.  pos / nuc[0 .. min(cap, *n_out)) are written and *n_out = off[n] is the true total.  The leaves run
 *   in launch windows; the _chunked twin (test hook) sets the leaves per window (0: default). */
typedef struct ugp_hp_group {
    uint32_t leaf;               /* BFS index of the first leaf of the group       */
    uint32_t count;              /* leaves with this haplotype                     */
    uint32_t size;               /* (position, allele) pairs of the haplotype      */
    uint32_t pad;
} ugp_hp_group;
typedef struct ugp_hp_info {
    uint64_t n_leaves;
    uint64_t n_groups;           /* runs of the sort, also when the call refuses   */
    uint64_t n_collisions;       /* leaves that differ from the leaf in front      */
    uint64_t n_duplicate;        /* nodes with a position twice                    */
    uint64_t n_visited;          /* entries read by the exact comparison           */
    uint32_t first_duplicate;    /* BFS index of the node                          */
    uint32_t pad;
} ugp_hp_info;
int ugp_haplotypes_attach(ugp_mat *mat, const ugp_tree_desc *tree);
int ugp_haplotype_groups(ugp_mat *mat, ugp_hp_group *out, uint64_t cap, uint64_t *n_out, ugp_hp_info *info);
int ugp_haplotype_groups_hashed(ugp_mat *mat, ugp_hp_group *out, uint64_t cap, uint64_t *n_out, ugp_hp_info *info, uint32_t hash_bits);
int ugp_haplotype_sets(ugp_mat *mat, const uint32_t *leaves /* BFS */, uint64_t n, uint64_t *off /* [n + 1] */, int32_t *pos, uint8_t *nuc,
                       uint64_t cap, uint64_t *n_out);
int ugp_haplotype_sets_chunked(ugp_mat *mat, const uint32_t *leaves, uint64_t n, uint64_t *off, int32_t *pos, uint8_t *nuc, uint64_t cap,
                               uint64_t *n_out, uint64_t chunk_leaves);
/* Bench hook: milliseconds of device time of the passes of ugp_haplotype_groups alone (no copies): the differences with their scan,
 * the two sorts of the leaves by fingerprint with the run heads, and the exact comparison; each the mean of `reps` runs after one
 * warm-up run. */
int ugp_haplotype_time(ugp_mat *mat, uint32_t reps, double *scan_ms, double *sort_ms, double *verify_ms);
/* RIPPLES (ripples/main.cpp): the options of :22-44 that the search reads. branch_len >= 1 and parsimony_improvement >= 0
 * (UGP_ERR_INVALID otherwise: the reference's size_t arithmetic of :445-453 is not reproduced for negative values). */
typedef struct ugp_ripples_opts {
    uint32_t branch_len;              /* -l: rows on each side of a breakpoint pair                         */
    int32_t min_range, max_range;     /* -r / -R: bounds of pos[j-1] - pos[i]                               */
    int32_t parsimony_improvement;    /* -p                                                                 */
    uint32_t num_descendants;         /* -n: candidate nodes have >= n nodes in their subtree (:280-289)    */
} ugp_ripples_opts;
/* One selected breakpoint pair of one branch, before the interval refinement of :608-666. */
typedef struct ugp_ripples_event {
    uint64_t branch;                  /* index into branches[]                                              */
    uint32_t i, j;                    /* the donor takes rows [i, j) of the branch's pruned sample          */
    uint32_t donor, acceptor;         /* BFS indices                                                        */
    uint32_t donor_count, acceptor_count;   /* Recomb_Node::parsimony: unmatched mutations in / out of range */
    int32_t donor_score, acceptor_score;    /* Recomb_Node::node_parsimony: pass-1 node_set_difference       */
    uint8_t donor_sibling, acceptor_sibling;   /* Recomb_Node::is_sibling ('y' = 1)                         */
    uint8_t pad[6];
} ugp_ripples_event;
/* Replaces main.cpp:280-289 (tree_num_leaves) and the per-branch setup: tables of `tree` (the handle's tree: same parent array)
 * and name_rank[k] = the rank of node k's identifier in std::string order (a permutation of 0 .. n-1; the donor / acceptor lists
 * sort by (count, name)).  Arrays are copied.  Two non-masked mutations at one position on one branch: UGP_ERR_UNSUPPORTED. */
int ugp_ripples_attach(ugp_mat *mat, const ugp_tree_desc *tree, const uint32_t *name_rank);
/* Replaces main.cpp:300-680 up to the refinement, for each branch of `branches` (BFS, any order, repeats allowed): the pruned
 * sample of the branch's root path (:68-90, :317-325), pass 1 (:343-377: mapper2_body(inp, true) over every node with
 * >= num_descendants subtree nodes), the unmatched-mutation filter and both node passes of every breakpoint pair (:383-575),
 * the sort / 1000-truncation and the donor-acceptor choice (:577-606).  Events come out in branch order, then pair order (i, then
 * j ascending), at most one per pair; out[0 .. min(cap, *n_out)) is written and *n_out is the true count.  is_sibling: the
 * reference sets node_has_unique only for nodes that tied or beat the running best, which depends on TBB's schedule; here
 * exactly the final ties carry their has_unique (a leaf always reads 1). */
int ugp_ripples(ugp_mat *mat, const ugp_ripples_opts *opts, const uint32_t *branches /* BFS */, uint64_t n, ugp_ripples_event *out,
                uint64_t cap, uint64_t *n_out);
/* bfs_of[k] = breadth-first index of the node at position k of `order` (how a caller maps its own node vector). */
int ugp_node_order(ugp_mat *mat, uint32_t order, uint32_t *bfs_of /* [n_nodes] */);
/* mask_out[k] = 1 for the nodes of the subtree of root_j that lie at most max_levels below it (merge.cpp:253-256). */
int ugp_subtree_mask(ugp_mat *mat, uint32_t order, uint32_t root_j, uint32_t max_levels, uint8_t *mask_out /* [n_nodes] */);

/* Device-resident variant (no PCIe in the timed path): upload once, place many
 * times.  `stream` is a hipStream_t (NULL = the default stream); d_out is a
 * device pointer to n_queries ugp_result records.  ugp_place_device is asynchronous
 * and STREAM-ORDERED on `stream`, like a kernel launch: it runs behind everything
 * queued on `stream` before it and in front of everything queued after it. */
int ugp_qset_upload(ugp_mat *mat, const ugp_queries *q, ugp_qset **out);
/* (A query set belongs to the handle it was uploaded for.  Sets with many rows per sample -- from 128 on average: the runs of N
 * of low-coverage samples -- also get one bit per (sample, tree site) on the device, about 3 KB per sample at 25,000 sites for
 * the tree and again for its coarse copy, from which every placement call builds its allele tiles.) */
void ugp_qset_destroy(ugp_qset *qs);
uint64_t ugp_qset_size(const ugp_qset *qs);
int ugp_place_device(ugp_mat *mat, ugp_qset *qs, void *d_out, void *stream);
/* Opt-in: consecutive ugp_place_device_overlapped calls on one handle overlap on the device -- up to d = ugp_pipeline_depth(mat)
 * of them at a time (internal streams, workspace sets; d = 3 by default: the small latency-bound kernels around the tree walk of one
 * batch run in the gaps of the others', and each walk takes its share of the resident wave slots; +15 % placements/s at 16,384
 * samples per call over two at a time, +65 % over one).  The price is a weaker ordering than a kernel launch has:
 *   - `stream` receives every call's completion, in call order: work queued on `stream` after call k sees its results;
 *   - call k runs behind the work that was on `stream` when call k - (d - 1) was made -- d - 1 CALLS OF LAG; work queued since
 *     sits behind the completion of a call that is still running, and waiting for it would serialise the calls.  (When no
 *     overlapped call is running any more, call k waits for everything on `stream`.)
 * Hence: cycle through d output buffers.  Whatever is queued on `stream` to read buffer A between call k (which wrote A) and call
 * k + 1 is finished before call k + d overwrites A.  Do not prepare d_out or the query set on `stream` right before the call and
 * expect the call to wait for it -- use ugp_place_device for that. */
int ugp_place_device_overlapped(ugp_mat *mat, ugp_qset *qs, void *d_out, void *stream);
/* How many overlapped calls the handle keeps on the device at a time (its workspace sets: 3 by default, 2..4 with
 * UGP_PIPELINE_DEPTH in the environment when the handle is made) = the number of output buffers to cycle through. */
int ugp_pipeline_depth(const ugp_mat *mat);

/* ugp_place_batch with several batches in flight: host buffers in, host buffers out, asynchronous.  The rows are copied out of
 * `q` before the call returns (pinned staging), `out` is written by ugp_job_wait.  At most ugp_pipeline_depth(mat) jobs per
 * handle may be outstanding (3 by default; batches of more than 32,768 samples or of 128 rows per sample and more: 2 -- one
 * call more fails until the oldest has been waited for); wait for them in the order they were started.
 * ugp_job_wait returns the call's status -- the row checks of ugp_place_batch surface here -- and frees the job.
 *   ugp_job *a, *b; ugp_place_batch_async(mat, &q0, r0, &a);
 *   for (i = 1; i < n; i++) { ugp_place_batch_async(mat, &q[i], r[i], &b); ugp_job_wait(a); a = b; }   ugp_job_wait(a);
 * keeps the device busy with the kernels of one batch while the next one's rows are on their way (two in flight; a ring of
 * ugp_pipeline_depth jobs keeps the device as busy as ugp_place_device_overlapped does: 11.8 M placements/s from host buffers to
 * host buffers at 16,384 samples per job on a 10M-node tree, against 12.5 M/s for inputs resident on the device). */
typedef struct ugp_job ugp_job;
int ugp_place_batch_async(ugp_mat *mat, const ugp_queries *q, ugp_result *out /* [n_queries], valid until ugp_job_wait */, ugp_job **job);
int ugp_job_wait(ugp_job *job);

/* ---- add mode: the tree changes between samples ------------------------------------------------------------------------
 * Default `usher` inserts every sample before it searches for the next (usher_common.cpp:310, the tree edits :652-765), and
 * the reference therefore re-expands and re-searches the whole tree per sample (:342).  An insertion changes very little:
 * it creates a leaf (and, for a sibling placement, an internal node) and rewrites the branch of best_node; the root-path
 * mutation set of every OTHER node -- hence its cost, eligibility and has_unique for any sample (usher_mapper.cpp:167-504) --
 * stays what it was.  This library keeps the flattened tree of ugp_mat_create on the device and takes the edits beside it:
 *
 *   ugp_mat_update   the caller reports the nodes it created or rewrote ("touched") as records: own mutations + the state of
 *                    the node's parent wherever that differs from the reference base.  Records of nodes that exist in the
 *                    flattened tree (flat_j != UINT32_MAX) also take that node OUT of the candidate set of every later
 *                    ugp_place_* / ugp_tied_nodes call on the handle: those calls then return the exact best score, tie count
 *                    and winner over the flattened nodes that are still what they were (winner by the leaf counts and order of
 *                    the flattened tree -- a caller whose tree has grown re-ranks the tie list itself).
 *   ugp_touched_*    score the live records against a batch of pending samples on the device: per sample the minimum cost
 *                    over the eligible records and the records that attain it.  The answer on the tree as it is NOW is the
 *                    merge of the two -- usher_amd/csrc/host/driver.cpp does exactly that, INTEGRATION.md 2a.
 * Records get ids 0, 1, 2 ... in the order they are handed over.  A node that is rewritten again gets a new record; the old
 * one is retired.  Needs a tree of fewer than 2^30 nodes (one bit of the 32-bit record streams marks an excluded node). */
#define UGP_T_LEAF   1u   /* the node is a leaf */
#define UGP_T_MASKED 2u   /* the node carries a masked mutation: `own` lists the mutations in front of it (usher_mapper.cpp:197-200) */
typedef struct ugp_touched {
    uint64_t n;                  /* records in this call                                                                       */
    const uint32_t *flat_j;      /* [n] index of the node in the tree given to ugp_mat_create; UINT32_MAX: created since       */
    const uint8_t *flags;        /* [n] UGP_T_*                                                                                */
    const uint32_t *n_path;      /* [n] how many of the record's entries describe the parent's state (they come first)         */
    const uint64_t *ent_off;     /* [n + 1] CSR into the entry arrays: the parent-state entries, then the own mutations        */
    const int32_t *pos;          /* [n_ent] position                                                                           */
    const uint8_t *allele;       /* [n_ent] parent-state entry: the state (one-hot, != ref); own mutation: the mutated allele  */
    const uint8_t *prev;         /* [n_ent] own mutation: the true parent state at pos (one-hot); parent-state entry: unused   */
    const uint8_t *ref;          /* [n_ent] reference base at pos (one-hot)                                                    */
} ugp_touched;
/* Appends `recs` (may be NULL / n = 0), retires the records listed in `retired` (ids of earlier calls), excludes the flattened
 * nodes named by the new records.  *first_id = id of the first new record. */
int ugp_mat_update(ugp_mat *mat, const ugp_touched *recs, const uint32_t *retired, uint64_t n_retired, uint32_t *first_id);
/* Begin scoring for a batch of pending samples: uploads their rows (checked like ugp_place_batch's), scores every live record. */
int ugp_touched_open(ugp_mat *mat, const ugp_queries *batch);
/* Records with id >= first_id against the samples first_sample .. end of the open batch, merged into the running results
 * (after ugp_mat_update: the samples in front of first_sample have been consumed already). */
int ugp_touched_score(ugp_mat *mat, uint32_t first_id, uint64_t first_sample);
/* One sample again from every live record (its list held retired records only). */
int ugp_touched_rescore(ugp_mat *mat, uint64_t sample);
/* Results of samples [first_sample, first_sample + n): best[i] = minimum cost over the eligible live records (INT32_MAX: none),
 * count[i] = how many attain it (true count), ids / has_unique [i * cap ..] = min(count, cap, 64) of them -- the device keeps 64
 * per sample, in no particular order; with cap < 64 the first `cap` of those it kept; the rest of a row is left as it was.  A
 * record retired after it entered a list is still listed: the caller knows which ids it retired. */
int ugp_touched_fetch(ugp_mat *mat, uint64_t first_sample, uint64_t n, uint32_t cap, int32_t *best, uint32_t *count, uint32_t *ids,
                      uint8_t *has_unique);

/* Per-kernel durations of the last ugp_place_* call on this handle, measured
 * with HIP events on the stream the kernels ran on (synchronises that stream). */
int ugp_get_timing(ugp_mat *mat, ugp_timing *out);
/* The same durations summed over every ugp_place_* call on this handle since the previous ugp_get_timing_sum (the other
 * fields are those of the last call); waits for the calls still in flight.  Lets a caller time a pipelined sequence of
 * ugp_place_device calls without synchronising after each of them. */
int ugp_get_timing_sum(ugp_mat *mat, ugp_timing *sum, uint32_t *n_calls);

/* Test hook: the third pruning bound's tables of 512-sample tile `tile` as the handle's most recent placement
 * call built them: cum_over / cum_under per block of 16 packed-stream words.  *n_blocks = entries per tile (0: that call did not
 * use the bound); with over == NULL only the count is returned.  Blocking; the caller checks `tile` against its own batch. */
int ugp_debug_bound3_tables(ugp_mat *mat, uint32_t tile, uint16_t *over, uint16_t *under, uint64_t cap, uint64_t *n_blocks);
/* Test hook: builds the third bound's tables from nibbles the caller supplies, as the tile builders would have left them:
 * useful[n_tiles][(n_sites + 7) / 8], one nibble per site (bit a: allele a is useful for the tile), 1..96 tiles.  Runs the three
 * table kernels into buffers of its own (never the ones a placement call reads) and returns, tile-major, over / under
 * [n_tiles][n_blocks] and the maxima l1 [n_tiles][ceil(n_blocks / 64)], l2 [..][ceil(that / 64)], l3 likewise.  *n_blocks = blocks per
 * tile; with every output NULL only that is returned.  Blocking.  UGP_ERR_UNSUPPORTED for a handle without event lists. */
int ugp_debug_bound3_build(ugp_mat *mat, const uint32_t *useful, uint32_t n_tiles, uint8_t *over, uint8_t *under, uint8_t *l1, uint8_t *l2, uint8_t *l3,
                           uint64_t *n_blocks);
/* Test hook: only the locality pre-pass of a batch, by method (0: the walk of the coarse tree, 1: the pass from the samples' own
 * rows, refused with UGP_ERR_UNSUPPORTED where a call would not take it).  Blocking.  cost / coarse_node: [n_queries]; kept_bfs
 * (optional, room for kept_cap): the BFS indices of the coarse tree's nodes, which coarse_node indexes. */
int ugp_debug_coarse_pass(ugp_mat *mat, ugp_qset *qs, int method, int32_t *cost, uint32_t *coarse_node, uint32_t *kept_bfs, uint64_t kept_cap, uint64_t *n_kept);
/* Test hook: the pre-pass of the handle's latest placement call -- 0: none, 1: the walk of the coarse tree, 2: from the samples' rows. */
int ugp_debug_last_prepass(const ugp_mat *mat);

/* Message for the last non-zero return on the calling thread. */
const char *ugp_last_error(void);

/* ---- MAT construction: Fitch-Sankoff over a batch of VCF sites ---------------
 * Replaces mapper_body::operator() (src/usher_mapper.cpp:6-161), which the VCF
 * reader runs once per site (src/mutation_annotated_tree.cpp:2108-2179) when a
 * MAT is built from a newick tree (`usher -t`).  All sites are assigned in one
 * call; the caller adds the returned mutations to its nodes (Node::add_mutation).
 * Cells of samples that are not in the tree never reach this call (the reader
 * keeps them as the samples' own mutation lists, usher_mapper.cpp:65-82). */
typedef struct ugp_sites {
    uint64_t n_sites;
    const uint8_t *ref;        /* [n_sites] one-hot reference allele (1,2,4,8) */
    const uint64_t *var_off;   /* [n_sites + 1] CSR into var_* */
    const uint32_t *var_node;  /* breadth-first index of the node the VCF column names (leaf or internal) */
    const uint8_t *var_nuc;    /* its allele mask 1..15 (15 = missing); cells equal to REF are simply absent */
} ugp_sites;
typedef struct ugp_fitch ugp_fitch;   /* result handle (host memory) */

/* `parent` is the breadth-first parent array of ugp_tree_desc (root first, parent[0] = UINT32_MAX).
 * The result lists every (site, node) whose assigned state differs from its parent's
 * (the root's parent state is REF), ordered by site, then node index. */
int ugp_fitch_sankoff(int device, uint64_t n_nodes, const uint32_t *parent, const ugp_sites *sites, ugp_fitch **out);
uint64_t ugp_fitch_count(const ugp_fitch *f);
int ugp_fitch_get(const ugp_fitch *f, uint32_t *site, uint32_t *node, uint8_t *par_nuc /* one-hot */, uint8_t *mut_nuc /* one-hot */);
void ugp_fitch_destroy(ugp_fitch *f);
/* ugp_fitch_sankoff keeps its device buffers (row storage of up to 16 GiB -- half of the free HBM if that is less --, sort and output buffers) in a per-device pool for the next
 * call; ugp_fitch_release(device) frees them -- e.g. when the MAT has been built and the same device goes on to place samples. */
void ugp_fitch_release(int device);

/* ---- test / tuning hooks (not part of the drop-in surface) ---------------- */

/* The tuning switches (UGP_* environment variables) are read ONCE, when a handle is created; no placement
 * call reads the environment.  A tool that sweeps switches on one handle re-reads them with this. */
int ugp_mat_reload_knobs(ugp_mat *mat);
/* 1: built with -DUGP_EXPERIMENTS (libusher_amd_exp.so: statistics build of the walk, UGP_STATS / UGP_TRACE /
 * UGP_SEED_PREV / UGP_SEED_CHECK / UGP_PHASE2_PACKED / UGP_KBEST_EXCLUSIVE); 0: the release library ignores those. */
int ugp_has_experiments(void);

/* ugp_mat_create with an explicit chunk size (nodes per DFS chunk), so small
 * fixtures exercise multi-chunk launches. */
int ugp_mat_create_chunked(const ugp_tree_desc *tree, int device, uint32_t chunk_nodes, ugp_mat **out);

/* Host-only view of the flattened tree (works without a GPU): the DFS record
 * stream and tables that ugp_mat_create uploads. */
typedef struct ugp_flat ugp_flat;
enum {
    UGP_FLAT_STREAM = 0,        /* uint32 */
    UGP_FLAT_PRE_STREAM = 1,    /* uint32 */
    UGP_FLAT_CHUNK_BODY_OFF = 2,/* uint32 [n_chunks+1] */
    UGP_FLAT_CHUNK_PRE_OFF = 3, /* uint32 [n_chunks+1] */
    UGP_FLAT_CHUNK_NODE_OFF = 4,/* uint32 [n_chunks+1] */
    UGP_FLAT_POS2SITE = 5,      /* int32  [max_pos+1] */
    UGP_FLAT_SITE_REF = 6,      /* uint8  [n_sites] */
    UGP_FLAT_RANK2BFS = 7,      /* uint32 [n_nodes] */
    UGP_FLAT_DFS2BFS = 8,       /* uint32 [n_nodes] */
    UGP_FLAT_MAX_SLOTS = 9,     /* count only */
    UGP_FLAT_STREAM8 = 10,      /* uint32: packed stream walked by the 8-samples-per-lane kernel */
    UGP_FLAT_PRE8_STREAM = 11,  /* uint32 */
    UGP_FLAT_CHUNK8_BODY_OFF = 12, /* uint32 [n_chunks+1] */
    UGP_FLAT_CHUNK8_PRE_OFF = 13,  /* uint32 [n_chunks+1] */
    UGP_FLAT_MAX_PATH_MUTS = 14, /* count only */
    UGP_FLAT_STREAM_T = 15,     /* uint32: tie stream walked by phase 2 (chunk bodies + pruning pseudo-records) */
    UGP_FLAT_CHUNK_T_OFF = 16,  /* uint32 [n_chunks+1] */
    UGP_FLAT_LDS_SLOTS = 17,    /* count only: saved-D slots the packed stream keeps on the fast path */
    UGP_FLAT_B3_GROUP_OFF = 18, /* uint32 [4][groups + 1]: third pruning bound, the four event lists of every group of 256 blocks of 16 packed-stream words */
    UGP_FLAT_B3_EVENTS = 19     /* uint32 [events]: 4 * site + allele (bits 23:0) | block within the group (31:24) */
};
int ugp_flat_create(const ugp_tree_desc *tree, uint32_t chunk_nodes, ugp_flat **out);
void ugp_flat_destroy(ugp_flat *flat);
int ugp_flat_get(const ugp_flat *flat, int which, const void **ptr, uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* USHER_AMD_H */
