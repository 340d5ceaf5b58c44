/*
 * ocn_hip.h — C ABI of libocn_hip.so, the MI355X (gfx950) implementation of OCN's
 * common-neighbour predictor hot path.
 *
 * The reference (qingpingmo/OCN) is pure Python: the boundary of this path is a Python
 * module API, and every entry below replaces the third-party native call
 * the reference makes at the cited file:line (paths relative to the reference root).
 * The Python mirror in ocn_amd/ binds these with ctypes.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller; nothing is allocated or freed
 *    inside the library and no entry synchronises the host (graph-capturable);
 *  - `stream` is a hipStream_t passed as void*; work is enqueued on it and the call returns;
 *  - CSR adjacency: rowptr int64 [n_rows+1], col int32 [nnz], columns ascending in a row;
 *  - candidate edges: int64 src[B], dst[B] (the reference's LongTensor tar_ei rows);
 *  - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *    OCN_E* code for argument errors.  Never throws.
 */
#ifndef OCN_HIP_H
#define OCN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history — 2: workspaces zero on entry / left zero, ocn_check_edges, ocn_zero_regions, ocn_cn_colsum_exact, walk prep /
 * group entries, dense block route, ocn_heads_fused; 3: ocn_cn_flags takes bit rows of T1, ocn_bitrows_from_csr;
 * 4: ocn_batch_prep, ocn_order_by_node_finish; 5: slot records (`rec`) from ocn_cn_flags to ocn_cn_gather;
 * 6: ocn_heads_fused on f16 hi/lo panels (ocn_heads_split_weight replaces ocn_linear_split_weight_chained).
 * 7: + ocn_coo_to_csr, ocn_wgrad, ocn_cn_gather_backward_det, ocn_gather_schedule; ocn_cn_flags gains `gcost`,
 *    ocn_cn_gather gains `perm` and `rowsum`.
 * 8: a scan whose workspace was not zero ends in OCN_SCAN_POISON totals and a status bit instead of a GPU trap; `status` is
 *    int32[4] for every intersection entry, word 3 the sticky error word; ocn_cn_weights_cn7 takes the Chebyshev diagonals,
 *    ocn_gather_schedule a segment; + ocn_cn_gather3_backward, ocn_cn_gather_backward_det_lists, ocn_ln_drop_relu_*.
 * 9: + ocn_heads_small_batch (ocn_heads_fused picks its small-batch form by the batch size; same bits), ocn_spgemm_bit_rows
 *    (ocn_cn_flags accepts rowptrT2 == NULL beside bitmapT2).  Later additions to 9 (backward-compatible): ocn_spmm_csr_max_arg,
 *    ocn_spmm_max_backward (max aggregation under autograd); ocn_spmm_csr's max mode takes the entry values (val);
 *    ocn_order_by_node_finish_rec, ocn_cn_flags_rec (slot records started by the prep pass); ocn_cn8_pool; ocn_cn_node_sums;
 *    ocn_row_diff_count / _fill, ocn_segment_topk (link recommendation); ocn_two_hop_diff_count / _fill (its candidates
 *    expanded from A, where A² is not stored); ocn_philox4x32, ocn_complement_count, ocn_sample_stage_cols,
 *    ocn_sample_complement_rows, ocn_sample_complement_pairs (structured negative sampling); ocn_csr_union_count / _fill,
 *    ocn_bitrows_insert_workspace_bytes, ocn_bitrows_insert (edge insertion into a resident graph); ocn_csr_minus_count /
 *    _fill, ocn_bitrows_remove_workspace_bytes, ocn_bitrows_remove (edge removal from a resident graph); ocn_spmm_csr_rows,
 *    ocn_rows_neighbourhood_workspace_bytes, ocn_rows_neighbourhood, ocn_bitlist_count / _fill (refreshing the node embeddings
 *    after an edge update: only the rows that can have changed); ocn_cn3_flags (the (A, A³) pass of cn6 from A and the bit rows
 *    of A², without a stored A³); ocn_cn_flags_pair_min_batch (the intersection pass takes two slots per wave at large batches;
 *    same bits); ocn_cn_pool_frozen (cn5 / cn7 pooled with a frozen column-weight table: intersection and weighted pooling in
 *    one pass); ocn_two_hop_sums_window_cols, ocn_two_hop_sums_fill (the 2-hop candidates with their cn / aa / ra path sums:
 *    the retrieval half of two-stage recommendation); ocn_cn_attribution (explaining a predicted link: the share of every
 *    common neighbour in the pooled vectors' part of a score); ocn_frontier_window_cols, ocn_frontier_count,
 *    ocn_frontier_sums_fill (frontier expansion with ordered path sums: chained, the candidates within three hops and their
 *    local path index); ocn_segment_rank (the place of held-out links among a source's candidates, in the order of
 *    ocn_segment_topk: ranking metrics); ocn_sample_two_hop_window_cols, ocn_sample_two_hop (hard negatives: draws from the
 *    2-hop candidate set that is served, selected in the expansion's LDS bitmap without listing the set); ocn_sddmm_csr (the sampled
 *    dense-dense product on the pattern of an encoder operator: the gradient of a layer with respect to its messages);
 *    ocn_cn_gather_pair_min_batch (the H = 256 pooling takes two slots per wave at large batches; same bits);
 *    ocn_rw_max_walks, ocn_rw_visits_count, ocn_rw_visits_fill (random-walk retrieval: a source's candidates and their visit
 *    counts from W walks of 2 or 3 steps, at a cost that does not depend on its degree); ocn_mips_max_m, ocn_mips_h_align,
 *    ocn_mips_workspace_bytes, ocn_mips_topm_i8 (embedding retrieval: the m largest int8 inner products of every query over all
 *    nodes, exact, on the integer matrix cores — a short list that is not bound to the graph neighbourhood);
 *    ocn_cn_flags_cover (the intersection pass with a certificate that T2 is the full A·A of a symmetric A: candidates that are
 *    stored entries of A read no T2; same bits); ocn_cn_gather_h16 (the pooling from a bf16 / f16 embedding table: half the
 *    bytes per row, fp32 sums, bit for bit ocn_cn_gather on the widened table); ocn_walk_hash (the walk route's Bloom and slot
 *    hashes on the host: tests build colliding node ids with the library's own arithmetic); OCN_REC_* / OCN_SCHED_* (names for
 *    the slot record's fields and the schedule's limits: macros only, no entry added or changed); ocn_cn_gather_cap (the
 *    pooling with at most `cap` sampled, reweighted rows per candidate: an unbiased estimate at a bounded cost; candidates
 *    within the cap bit for bit ocn_cn_gather's); ocn_cn_gather_q8 (the pooling, exact or capped, from the int8 rows and row
 *    scales a retrieval index keeps: one resident image for retrieval and scoring, a quarter of the bytes per row, bit for bit
 *    ocn_cn_gather / ocn_cn_gather_cap on the dequantised table); ocn_segment_keep_best (the m best entries of every segment
 *    as a set, in position order, for any m: short lists beyond ocn_segment_topk_max_k()). */
#define OCN_ABI_VERSION 9
#define OCN_EINVAL (-1)   /* null pointer / negative size / unsupported combination */
#define OCN_ECAP   (-2)   /* reported through the device status word: flags capacity too small */

/* Device status words of a candidate batch: int32[4].  [0] = error bits of THIS batch (cleared by the caller / by
 * ocn_batch_prep's resets with the batch's other scratch), [1], [2] = work-item tickets of the walk route, [3] = the same
 * error bits, STICKY: the library only ever ORs into it; the caller clears it when it has read it, so a scoring loop can
 * check a whole split with one read (ocn_amd.pipeline does) instead of one host sync per batch. */
#define OCN_ST_CAP  1     /* off[B] > flags_cap: the flag buffer is too small (nothing is written past the cap) */
#define OCN_ST_SCAN 2     /* the batch's offsets come from a scan that gave up (OCN_SCAN_POISON): its workspace was not zero */
#define OCN_SCAN_POISON (-1)   /* out[n] of a scan entry whose workspace was not zero on entry (see ocn_scan_workspace_bytes) */

/* bits of a CN flag byte */
#define OCN_F_CN1 1u      /* neighbour k of src is in adj1-target row of dst  (cn1 entry) */
#define OCN_F_CN2 2u      /* neighbour k of src is in adj2-target row of dst  (cn2 entry) */

int ocn_abi_version(void);

/* Scratch bytes the scan entries need for `n` items.  The workspace must be ZERO when first handed to the library
 * (the caller zeroes it once, when it allocates it); every entry leaves it zero again, so it can be reused from call
 * to call — inputs beyond one tile are scanned by a single launch whose tiles chain through this state.  A workspace
 * that is NOT zero breaks the chain (two launches in flight on one workspace, a buffer never cleared).  The launch then
 * neither hangs nor traps: after a bounded wait the tiles that cannot be chained write ZERO offsets for their items and
 * the total out[n] becomes OCN_SCAN_POISON (< 0).  Consumers test the total and do not trust the offsets: ocn_cn_flags /
 * ocn_cn_walk_flags raise OCN_ST_SCAN in their status words and treat the batch as empty (zero counts, empty slot
 * records), ocn_order_by_node_finish / ocn_class_order fall back to batch order (a correct order, only slower), and a
 * caller that reads a total on the host (nnz of a product, the flag capacity) sees a negative number.  Detection is
 * best effort: the contract (ZERO on entry, one launch at a time per workspace) stays the caller's. */
int64_t ocn_scan_workspace_bytes(int64_t n);

/* Zero up to 8 device arrays (4-byte aligned, byte counts multiples of 4) with one launch: the per-batch reset of
 * the histogram / counters / status words. */
int ocn_zero_regions(void* const* ptrs, const int64_t* bytes, int32_t n, void* stream);

/* off[e] = sum_{e'<e} deg_A(src[e']), off[B] = total: where each batch row starts in the
 * flag buffer.  Replaces the row bookkeeping of SparseTensor.__getitem__ (utils.py:256). */
int ocn_edge_offsets(const int64_t* rowptrA, const int64_t* src, int64_t B,
                     int64_t* off, void* workspace, void* stream);

/* bad[0] |= 1 when any src[e] is outside [0, n_src) or any dst[e] outside [0, n_dst) (bad[0] is NOT
 * cleared here).  The reference's row selection raises IndexError for such an id
 * (SparseTensor.__getitem__ -> index_select, utils.py:256-257); the kernels below would read out of
 * bounds instead, so the Python mirror runs this check first and raises the same exception. */
int ocn_check_edges(const int64_t* src, const int64_t* dst, int64_t B, int64_t n_src, int64_t n_dst,
                    int32_t* bad, void* stream);

/* A processing order for a candidate batch: order[] = the batch rows counting-sorted by the node id
 * in `node` (arbitrary order among equal ids).  Visiting rows with the same / nearby source node
 * together lets the rows they share be served from L2; it never changes a result.
 * workspace: ocn_order_workspace_bytes(n_nodes) bytes of device scratch, ZERO when first handed over and left zero
 * (per-node counters that each batch row clears again, and the scan state). */
int64_t ocn_order_workspace_bytes(int64_t n_nodes);
int ocn_order_by_node(const int64_t* node, int64_t B, int64_t n_nodes, int64_t* order, void* workspace,
                      void* stream);

/* One launch for everything in front of the intersection pass of a large batch: the flag offsets (ocn_edge_offsets), the
 * counting phase of ocn_order_by_node (order_workspace, or NULL: no processing order) and the batch's resets
 * (ocn_zero_regions' arguments) — the two latter ride on extra workgroups of the scan's launch.  Follow with
 * ocn_order_by_node_finish (scan of the counters + scatter) for the order itself.  Workspaces: ZERO on entry, left zero. */
int ocn_batch_prep(const int64_t* rowptrA, const int64_t* src, int64_t B, int64_t* off /* [B+1] */, void* scan_workspace,
                   int64_t n_nodes, void* order_workspace /* or NULL */, void* const* zero_ptrs, const int64_t* zero_bytes,
                   int32_t n_zero, void* stream);
int ocn_order_by_node_finish(const int64_t* node, int64_t B, int64_t n_nodes, int64_t* order, void* workspace,
                             void* stream);
/* ocn_order_by_node_finish for the pattern route's intersection pass: the scatter that gives a batch row its slot also
 * starts the slot's record (laid out under ocn_cn_flags `rec`): words 0 - 2 complete, word 3 = off[e] with no bit above it
 * (`off` as ocn_batch_prep / ocn_edge_offsets left it, on the same stream).  ocn_cn_flags_rec then starts every slot from
 * that one 32-byte load. */
int ocn_order_by_node_finish_rec(const int64_t* node /* src */, const int64_t* dst, const int64_t* rowptrA,
                                 const int64_t* off, int64_t B, int64_t n_nodes, int64_t* order, uint64_t* rec /* [B][OCN_REC_WORDS] */,
                                 void* workspace, void* stream);

/* Forward work-item offsets of the walk route: out[slot] = number of items of the earlier processing
 * slots, out[B] = number of items.  A batch row's items are groups of consecutive chunks of
 * ocn_walk_chunk() neighbours of its source; with nds (ocn_neighbor_degree_sum, or NULL) the group
 * size adapts so that an item sweeps a bounded number of elements — pass the SAME nds to
 * ocn_cn_walk_flags. */
int ocn_chunk_offsets(const int64_t* rowptrA, const int64_t* nds /* or NULL */, const int64_t* src,
                      const int64_t* order, int64_t B, int64_t* out, void* workspace, void* stream);

/* Class-major processing order for the MLP heads.  A candidate with no cn1 (cn2) entry has an all-zero
 * pooled xcn1 (xcn2), and a zero row through `xcn1lin` is the same constant vector for every such
 * candidate: sorted by class = (cnt1 > 0, cnt2 > 0) — 3 both, 2 cn1 only, 1 cn2 only, 0 none; stable, so
 * the order inside a class is that of `order_in` (or batch order) — the heads run on contiguous row
 * ranges and skip the rest (62 % / 47 % of a collab-shaped evaluation batch have no cn1 / cn2 entry).
 * order_out[slot] = batch row, inv_out[batch row] = slot; ranges[OCN_CLASS_RANGES][2] = {begin, end} of
 *   0: cn1 > 0   1: both   2: cn2 only   3: any   4: none   5: cn1 only   6: all rows
 * (device-resident: OcnLinearGroup.row_range points into it, no host sync).  prefix: int64[B+1] scratch;
 * workspace: ocn_scan_workspace_bytes(B). */
#define OCN_CLASS_RANGES 7
int ocn_class_order(const int32_t* cnt1, const int32_t* cnt2 /* or NULL */, const int64_t* order_in /* or NULL */,
                    int64_t B, int64_t* order_out, int64_t* inv_out, int64_t* ranges, int64_t* prefix,
                    void* workspace, void* stream);

/* What the intersection pass hands to the pooling.  The slot record (laid out under ocn_cn_flags `rec`; the kernels pack
 * and unpack it in ocn_amd/csrc/slot_rec.h and nowhere else): */
#define OCN_REC_WORDS      4    /* 64-bit words per slot */
#define OCN_REC_LEN_SHIFT 40    /* word 2: row start below, row length from this bit */
#define OCN_REC_FULL2_BIT 61    /* word 3: flag offset below; cnt2 == row length > 0 */
#define OCN_REC_HAS1_BIT  62    /* word 3: cnt1 > 0 */
#define OCN_REC_HAS2_BIT  63    /* word 3: cnt2 > 0 */
/* ... and the schedule (ocn_cn_flags `gcost`, ocn_gather_schedule): a group is OCN_SCHED_GROUP consecutive slots — a
 * workgroup of the intersection pass and of the H = 256 pooling; a schedule exists where every one of the OCN_SCHED_EIGHTHS
 * XCDs gets the same number of whole groups, at most OCN_SCHED_MAX_EIGHTH of them (16-bit ranks of the counting sort). */
#define OCN_SCHED_GROUP      4
#define OCN_SCHED_EIGHTHS    8
#define OCN_SCHED_MAX_EIGHTH 65535

/* Exclusive scan of int32 counts into int64 offsets (out[n] = total). */
int ocn_scan_i32(const int32_t* in, int64_t n, int64_t* out, void* workspace, void* stream);

/* The intersection: utils.adjoverlap -> spmoverlap_ (utils.py:162-183, 248-285), both calls
 * of a batch fused.  For edge e=(i,j) and the p-th neighbour k of i in A:
 *   flags[off[e]+p] = [k in T1 row j] | [k in T2 row j] << 1
 * cnt1[e] / cnt2[e] = |cn1_e| / |cn2_e| (the integer CN counts), and the per-column
 * histograms are accumulated (cn.sum(dim=0), model.py:2261,3114): hist[k] = {packed, walks}
 * with packed = n1 | n2 << 21 | n_union << 42 (one 64-bit atomic per CN entry) and walks = 0
 * here; must be zero on entry; B < 2^21.  T2 may be NULL (single adjoverlap call).
 * bitmapT2: optional dense bit rows of T2 (row j at bitmapT2 + j*bm_stride_words, bit k = column k;
 * written by ocn_spgemm_pattern_count): membership in the long A² row becomes one probe.
 * rec (or NULL): THE SLOT RECORD — per processing SLOT OCN_REC_WORDS 64-bit words (32 bytes, 16-byte aligned):
 *   word 0: the batch row e = order[slot]
 *   word 1: src[e] | dst[e] << 32                                  (node ids < 2^31)
 *   word 2: start of N(src) in colA | its length << OCN_REC_LEN_SHIFT      (nnz < 2^40)
 *   word 3: off[e] | (cnt2 == length > 0) << OCN_REC_FULL2_BIT | (cnt1 > 0) << OCN_REC_HAS1_BIT | (cnt2 > 0) << OCN_REC_HAS2_BIT
 * (bit OCN_REC_FULL2_BIT: every position of the source row is a cn2 entry — ocn_cn_gather's `rowsum` shortcut reads it.)
 * ocn_cn_gather given the same `rec` reads it instead of walking order -> src / dst / off / counts -> rowptr (one
 * dependent load in front of its first gather instead of three).  ocn_order_by_node_finish_rec starts a record (words
 * 0 - 2, word 3 = the bare off[e]); this pass finishes it.
 * gcost (or NULL): int32[ceil(B / OCN_SCHED_GROUP)]: per group of OCN_SCHED_GROUP consecutive processing slots the largest
 * number of cn1 + cn2 entries one of its candidates has — what the group will cost the pooling; see ocn_gather_schedule.
 * bitmapT1: the same for T1 (ocn_bitrows_from_csr; small dense graphs); rowptrT1 / colT1 may then be NULL.
 * status: device int32[4] (above): OCN_ST_CAP if off[B] > flags_cap (nothing is written past the cap), OCN_ST_SCAN if
 * off[B] is OCN_SCAN_POISON; both also ORed into the sticky word status[3].
 * order (here and below): optional permutation of 0..B-1 giving the order in which the batch rows
 * are PROCESSED (e.g. sorted by src so that rows sharing neighbourhoods meet in L2); every output
 * stays indexed by the batch row.  NULL = batch order. */
int ocn_cn_flags(const int64_t* rowptrA, const int32_t* colA,
                 const int64_t* rowptrT1, const int32_t* colT1,
                 const int64_t* rowptrT2, const int32_t* colT2,
                 const uint32_t* bitmapT1 /* or NULL */, int64_t bm1_stride_words,
                 const uint32_t* bitmapT2 /* or NULL */, int64_t bm_stride_words,
                 const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                 int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap,
                 uint64_t* hist /* [n_cols][2] */, int32_t* cnt1, int32_t* cnt2,
                 int32_t* status, uint64_t* rec /* [B][OCN_REC_WORDS] or NULL */, int32_t* gcost /* [ceil(B/OCN_SCHED_GROUP)] or NULL */, void* stream);
/* The same pass behind ocn_order_by_node_finish_rec: `order` and `rec` are required, the records (ocn_cn_flags `rec`) arrive
 * started — words 0 - 2 and the bare offset — and leave as ocn_cn_flags leaves them; src / dst / rowptrA are then not read per slot.  Every
 * output is identical to ocn_cn_flags' on the same arguments. */
int ocn_cn_flags_rec(const int64_t* rowptrA, const int32_t* colA,
                     const int64_t* rowptrT1, const int32_t* colT1,
                     const int64_t* rowptrT2, const int32_t* colT2,
                     const uint32_t* bitmapT1 /* or NULL */, int64_t bm1_stride_words,
                     const uint32_t* bitmapT2 /* or NULL */, int64_t bm_stride_words,
                     const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                     int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap,
                     uint64_t* hist /* [n_cols][2] */, int32_t* cnt1, int32_t* cnt2,
                     int32_t* status, uint64_t* rec /* [B][OCN_REC_WORDS] */, int32_t* gcost /* [ceil(B/OCN_SCHED_GROUP)] or NULL */, void* stream);
/* Either of the two (rec_in != 0: ocn_cn_flags_rec) with a certificate on T2.  t2_cover != 0 is the caller's word that T2 —
 * bit rows and CSR alike — is the FULL pattern of A·A and that A (rowptrA / colA, rows sorted) equals its transpose.  Then a
 * candidate (i, j) that is a stored entry of A has every neighbour k of i in T2 row j (the wedge j - i - k), and its cn2
 * flags are set without reading T2: no probe, no search.  Whether j is in N(i) is read off the source row the slot loads
 * anyway (rows of up to 4096 entries; longer ones read T2 as before).  Every output is what t2_cover == 0 leaves whenever
 * the certificate is true; a false one yields cn2 flags T2 does not hold.  Ignored without T2. */
int ocn_cn_flags_cover(const int64_t* rowptrA, const int32_t* colA,
                       const int64_t* rowptrT1, const int32_t* colT1,
                       const int64_t* rowptrT2, const int32_t* colT2,
                       const uint32_t* bitmapT1 /* or NULL */, int64_t bm1_stride_words,
                       const uint32_t* bitmapT2 /* or NULL */, int64_t bm_stride_words,
                       const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                       int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap,
                       uint64_t* hist /* [n_cols][2] */, int32_t* cnt1, int32_t* cnt2,
                       int32_t* status, uint64_t* rec /* [B][OCN_REC_WORDS] or NULL */, int32_t* gcost /* [ceil(B/OCN_SCHED_GROUP)] or NULL */,
                       int32_t rec_in, int32_t t2_cover, void* stream);

/* The pygho route get_cn1_cn2 (NeighborOverlap_large_ppa.py:147-173, NeighborOverlapCitation2.py:
 * 78-104) without forming Ej·A: cn1 = N(i) ∩ N(j) as above; cn2[e,k] = |N(k) ∩ N(j)| (number of
 * 2-walks j -> k) for k in N(i), kept where > 0.  wc[off[e]+p] receives the walk count, hist[k]
 * additionally accumulates walks = sum of the counts of column k; cnt2[e] = number of non-zero
 * entries of cn2 row e.  Work is cut into items of ocn_walk_chunk() neighbours of i (chunk_off from
 * ocn_chunk_offsets), so hub source nodes spread over many workgroups; cnt1 / cnt2 must be ZERO on
 * entry (a row's items add into them).  `status`: words [0] .. [2] ZERO on entry: [0] receives the
 * error bits as for ocn_cn_flags, [1] and [2] are the work-item ticket counters of the two sweeps, [3] the sticky word.
 * Under OCN_ST_CAP (off[B] > flags_cap) a batch row is written whole or not at all: flags and wc of a row with
 * off[e] + deg(src[e]) <= flags_cap are exact, the flags of every other row are left as they were, and so is its wc —
 * except that with nds the whole of wc below the cap is cleared first (the reverse sweep adds into it).  cnt1, cnt2 and
 * hist stay complete for the rows swept from the source's side (and for those of ocn_cn_walk_group), written or not.  A
 * row that does not fit and that walk_reverse sends to the target's side (its counts live in wc) reports no cn2 entry:
 * cnt1[e] and the n1 column of hist are complete, cnt2[e] is 0 and hist receives neither n2 nor walks from it (n_union
 * counts its cn1 entries). */
int32_t ocn_walk_chunk(void);
int ocn_cn_walk_flags(const int64_t* rowptrA, const int32_t* colA, const int64_t* nds /* or NULL */,
                      const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                      const int64_t* chunk_off, const int64_t* rev_off /* NULL iff nds is */, const int64_t* off,
                      int64_t max_row_len /* unused (kept for the ABI): the LDS copy of the probed row is fixed at 4096 entries */,
                      uint8_t* flags, int32_t* wc, int64_t flags_cap,
                      uint64_t* hist /* [N][2] */, int32_t* cnt1, int32_t* cnt2,
                      int32_t* status, void* stream);

/* Two-sided enumeration of the same walk counts: cn2[e,k] is the number of 2-walks j -> m -> k, which
 * can be swept from i's side (Σ_{k∈N(i)} deg k elements) or from j's side (Σ_{m∈N(j)} deg m).  With
 * nds[v] = Σ_{u∈N(v)} deg u (ocn_neighbor_degree_sum, once per adjacency) and rev_off = exclusive scan
 * of the reverse work items per batch row (ocn_walk_rev_offsets; 0 for rows swept forward),
 * ocn_cn_walk_flags sweeps each batch row from its cheaper endpoint; results are identical (integer
 * counts).  The pygho reference always expands from j (spspmm(Ej, 1, adj, 0)). */
int ocn_neighbor_degree_sum(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t* out,
                            void* stream);
int ocn_walk_rev_offsets(const int64_t* rowptrA, const int64_t* nds, const int64_t* src, const int64_t* dst,
                         const int64_t* order, int64_t B, int64_t* out /* [B+1] */, void* workspace,
                         void* stream);

/* Small batches of the walk route (B <= ocn_walk_prep_max_batch(): the ppa / citation2 drivers use 2048) — everything in
 * front of the walk kernels in ONE single-workgroup launch: order[] = a permutation of the batch rows in which the rows of
 * one source are contiguous (the sources in the order of their slots in a hash table, a source's rows in whatever order the
 * atomics gave them: neither is sorted, and no consumer needs more than the contiguity); off =
 * flag offsets (as ocn_edge_offsets); groups = runs of equal source cut into pieces of 64 (g_head[g] = first slot of
 * group g, g_head[n_groups] = B, meta[0] = n_groups); the members of a group whose target has at most 512 neighbours go
 * to the shared sweep ocn_cn_walk_group if their targets' rows sum to at most 4096 entries — if at least `min_share`
 * of them do (g_active[slot]; g_item_off = exclusive scan of the group's work items, one per meta[2] x 64 neighbours of the
 * source) —, every other candidate keeps its per-candidate work items in chunk_off / rev_off (as ocn_chunk_offsets /
 * ocn_walk_rev_offsets; 0 for the candidates of the shared sweep); cnt1, cnt2, status[0..2], scal[4] are cleared.  meta: int32[4] ([1] = the shared sweep's ticket).  rev_off NULL iff nds is.
 *
 * ocn_cn_walk_group: the rows N(k), k in N(i), that a candidate (i, j) sweeps for cn2[e,k] = |N(k) n N(j)| are the same
 * for every candidate with source i (the MRR layout scores 1000 negatives per source, NeighborOverlapCitation2.py:
 * 248-254): they are swept once per group, each element probed against ONE hash table (node -> 64-bit mask of the
 * group's targets it neighbours).  Same outputs as ocn_cn_walk_flags, for the candidates of the shared groups; run it
 * after ocn_cn_walk_flags of the same batch (which handles the others and zeroes wc). */
int32_t ocn_walk_prep_max_batch(void);
/* The hashes of the walk route, computed on the host by the functions the kernels call.  which = 0: bit of `node` in the
 * Bloom bitmap of the per-candidate sweeps (0 .. 2^17 - 1); 1: its bit in the shared sweep's bitmap (0 .. 2^17 - 1); 2: its
 * home slot in the shared sweep's key table and in ocn_walk_prep's source table (0 .. 8191; both probe linearly and wrap).
 * Another `which`: OCN_EINVAL.  For tests that must construct Bloom false positives and probe chains across the wrap. */
int32_t ocn_walk_hash(int32_t which, int32_t node);
int ocn_walk_prep(const int64_t* rowptrA, const int64_t* nds /* or NULL */, const int64_t* src, const int64_t* dst,
                  int64_t B, int32_t min_share, int64_t* order, int64_t* off, int64_t* chunk_off,
                  int64_t* rev_off /* NULL iff nds is */, int32_t* g_head /* [B+1] */, int64_t* g_item_off /* [B+1] */,
                  int32_t* g_active /* [B]: slot goes to the shared sweep */, int32_t* meta, int32_t* cnt1,
                  int32_t* cnt2, int32_t* status, int32_t* scal, void* stream);
int ocn_cn_walk_group(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                      const int64_t* order, int64_t B, const int32_t* g_head, const int64_t* g_item_off,
                      const int32_t* g_active, int32_t* meta, const int64_t* off, uint8_t* flags, int32_t* wc,
                      int64_t flags_cap, uint64_t* hist, int32_t* cnt1, int32_t* cnt2, void* stream);

/* Per-column weights, written IN PLACE over hist (uint64[N][2] -> float[N][4]) as
 *   {w1, t, inv2, 0}: a cn1 entry pools with w1; a union entry whose cn2 value is c (1.0 for the
 *   pattern route, the walk count for the valued route) pools into xcn2 with
 *   (c*[in cn2] - t*[in cn1]) * inv2.
 * cn5 (model.py:2261-2272, 2352-2413): w1 = 1/S1 (0 if S1 < 2); scale = max w1 over cn1
 * entries; nip = innerprod/scale (scale>0); t = nip*w1; S2 = column sums of cn2 - nip*ncn1 over
 * the union pattern (0 -> 1); inv2 = 1/S2.  `innerprod` is a device float[1] (the module buffer);
 * `scalars` is the statistics word of ocn_cn5_column_stats — run that entry first whenever innerprod may be
 * non-zero; for innerprod == 0 (a fresh model) nip is 0 whatever the scale, and zeroed scalars suffice;
 * `valued` != 0 for walk-count cn2.
 * cn7 (model.py:3114-3126, 3186-3209): w1 = 1/S1, `sum_fill` where S1 < 2; cn2 raw ->
 * {w1, 0, 1, 0}.  diag1 / diag2 (or NULL = ones): the Chebyshev diagonals diag(T_k(linspace(-1, 1, N))) of
 * evaluate_polynomial (model.py:2958-3019) that the reference multiplies the normalised cn1 (:3141-3165) and the raw cn2
 * (:3186-3209) by — one fp32 product per entry: {w1 * diag1[c], 0, diag2[c], 0}.  The reference hard-wires k = 0. */
int ocn_cn_weights_cn5(uint64_t* hist, int64_t N, const float* innerprod, int32_t* scalars,
                       int32_t valued, const float* s2_exact /* or NULL: closed form from the counts */, void* stream);
int ocn_cn_weights_cn7(uint64_t* hist, int64_t N, float sum_fill, const float* diag1 /* [N] or NULL */,
                       const float* diag2 /* [N] or NULL */, void* stream);

/* scalars[0] (zero before the first call of a batch; idempotent afterwards) = the batch's scale statistic of
 * model.py:2370-2375: 0 = empty union, -1 = no column with S1 >= 2, else min{S1 >= 2} - INT_MAX - 1. */
int ocn_cn5_column_stats(const uint64_t* hist, int64_t N, int32_t* scalars, void* stream);

/* Order-exact column sums for a non-zero `innerprod` (every trained checkpoint).  The reference forms
 * S2[c] = sum_e v[e,c], v = cn2 - nip*ncn1 on the union pattern, with index_add_ over the coalesced COO
 * (model.py:2405-2406): one fp32 add per entry, in ascending batch-row order; where colsum(cn2) ~ nip the
 * result depends on that order.  This entry transposes the union pattern of the batch into
 * per-column lists of flag positions (count -> scan -> fill -> per-column sort: positions ascend with the batch
 * row) and adds each column's values sequentially in fp32: s2[c] is bit for bit the reference's sum (before its
 * `== 0 -> 1` fix-up); pass it to ocn_cn_weights_cn5 / _cn6 as s2_exact.  Must run BEFORE the weights entry
 * (hist still holds the counts).  cn6 (flagsB = the cn3 flags of the (A, A^3) pass, s3 != NULL): additionally
 * s3[c] = column sums of cn3 - nip*ncn1 - nip*ncn2' over the three-way union (model.py:2895-2913).
 * wc: walk counts of the valued route or NULL.  flags_cap < 2^32.  scalars as for ocn_cn5_column_stats.
 * s2_init (or NULL = zeros; cn5 only): the running sums of the EARLIER rows of an edge-sharded batch — rank r of
 * ocn_amd/dist.py continues the chains rank r-1 left off (the global batch's rows ascend with the rank), so
 * the last rank ends with the single-device sums; hist must then hold the all-reduced (global) counts, the
 * entry counts of this shard are taken from the flags.
 * workspace: ocn_cn_colsum_workspace_bytes(N, flags_cap) bytes of device scratch. */
int64_t ocn_cn_colsum_workspace_bytes(int64_t N, int64_t flags_cap);
int ocn_cn_colsum_exact(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, int64_t B,
                        const int64_t* off, const uint8_t* flagsA, const uint8_t* flagsB /* or NULL */,
                        const int32_t* wc /* or NULL */, int64_t flags_cap, const uint64_t* hist /* [N][2], counts */,
                        int64_t N, const float* innerprod, int32_t* scalars, const float* s2_init /* [N] or NULL */,
                        float* s2 /* [N] */, float* s3 /* [N], iff flagsB */, void* workspace, void* stream);

/* The pooling: spmm_add(ncn1, x), spmm_add(ncn2, x) and x[i]*x[j] (model.py:2426-2429,
 * 3213-3216) in one pass.  xcn1[e] = sum_{k in cn1_e} w1[k] h[k]; xcn2[e] = sum over the
 * union pattern as above; xij[e] = h[i] (.) h[j]; entries in ascending column order, fp32
 * multiply then add.  wc = per-neighbour cn2 values of the walk route or NULL (all 1.0).
 * h is [N][H] row-major fp32; outputs [B][H].  max_row_len = longest row of A (upper bound):
 * batch rows whose source row exceeds 1024 entries (hubs) are pooled by a whole workgroup — or, for narrow embeddings
 * in a large batch, a wave — of their own: the other lanes fetch, ONE wave adds, so those rows keep the strictly
 * sequential ascending-column sum as well.  out_row (or NULL): batch row e is written to row
 * out_row[e] of the three outputs (ocn_class_order's inv_out: class-major rows for the heads).
 * cnt1 / cnt2 (or NULL): the per-row CN counts of the intersection pass; a row with neither kind of
 * entry is not walked at all, and with out_row the xcn1 / xcn2 rows the class-major heads never read
 * (no cn1 entry; no entry at all) are not written.
 * rec (or NULL): the finished slot records of the intersection pass (laid out under ocn_cn_flags `rec`); order, src, dst,
 * off and the counts are then not read per slot.  perm (or NULL): ocn_gather_schedule's visiting order of the groups.
 * rowsum (or NULL; pattern route with the cn7 weights only — the caller's promise that every cn2 entry has weight
 * exactly 1 and no cn1 correction): [N][H] rows (A h)[i] = sum_{k in N(i)} h[k] in ascending column order
 * (ocn_spmm_csr, mode sum).  A candidate whose WHOLE source row is cn2 (cnt2[e] = row length: the target's A^2 row
 * holds every neighbour of the source — ogbl-ddi, whose A^2 is full) has xcn2[e] = rowsum[src[e]], the same additions in
 * the same order, so the row is copied instead of summed again for every candidate of that source; only its cn1 entries
 * are gathered. */
int ocn_cn_gather(const int64_t* rowptrA, const int32_t* colA,
                  const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                  const int64_t* off, const uint8_t* flags, const int32_t* wc,
                  const float* weights /* [N][4] */, const float* h, int32_t H, int64_t max_row_len,
                  float* xcn1, float* xcn2, float* xij, const int64_t* out_row,
                  const int32_t* cnt1, const int32_t* cnt2, const uint64_t* rec /* or NULL */,
                  const int32_t* perm /* ocn_gather_schedule's, or NULL */, const float* rowsum /* or NULL */,
                  void* stream);
/* The pooling from a half-precision embedding table.  h16 is [N][H] row-major 2-byte elements: bf16 (fmt = 0) or IEEE f16
 * (fmt = 1); every other argument means what it means for ocn_cn_gather, and the outputs are fp32 [B][H].  Both widenings are
 * exact, the entry weights, the accumulators and the order are ocn_cn_gather's (each term one fp32 multiply, then one add,
 * ascending column order, strictly sequential for EVERY row length — a hub row is walked by the same lane group as any other),
 * and so are the skip rules (cnt1 / cnt2 / rec / out_row).  Hence xcn1, xcn2 and xij are bit for bit what ocn_cn_gather
 * leaves for the same table widened to fp32.  There is no `rowsum`: the shortcut wants an fp32 A h, and it adds the same
 * numbers in the same order, so leaving it out changes no bit.  max_row_len is accepted and not used (one form).  rec / perm
 * (the slot records laid out under ocn_cn_flags `rec`, ocn_gather_schedule's order) change the processing order only.  No allocation, no global state, no host synchronisation: the launch can be captured.
 * H in {16, 32, 64, 128, 256, 512}; h16 must be 16-byte aligned.  NULL required pointers (rowptrA, src, dst, off, weights, h16,
 * the outputs), B < 0, another H, fmt outside {0, 1}: OCN_EINVAL before any HIP call.  B == 0 returns 0. */
int ocn_cn_gather_h16(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                      const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flags, const int32_t* wc,
                      const float* weights /* [N][4] */, const void* h16 /* [N][H], 2-byte elements */,
                      int32_t fmt /* 0 = bf16, 1 = f16 */, int32_t H, int64_t max_row_len, float* xcn1, float* xcn2,
                      float* xij, const int64_t* out_row, const int32_t* cnt1, const int32_t* cnt2,
                      const uint64_t* rec /* or NULL */, const int32_t* perm /* or NULL */, void* stream);
/* The CAPPED pooling: ocn_cn_gather with at most `cap` embedding rows per candidate, chosen by a deterministic stratified
 * sample of the candidate's common-neighbour entries and reweighted so that xcn1 / xcn2 are unbiased estimates of
 * ocn_cn_gather's.  Every argument up to `perm` means what it means for ocn_cn_gather (fp32 table; there is no `rowsum`).
 * For candidate e = (i, j), q = off[e] + p over the positions p of row N(i): the MEMBERS are the positions with
 * flags[q] != 0, ranked r = 0 .. u - 1 in ascending p; d = cap.
 *   u <= d: every member is selected with multiplier s = 1.
 *   u >  d: stratum t = 0 .. d - 1 holds the ranks [lo_t, lo_{t+1}), lo_t = ceil(t u / d) (so t(r) = floor(r d / u), and
 *           the size s_t = lo_{t+1} - lo_t is floor(u / d) or ceil(u / d)); its one selected rank is
 *           lo_t + floor(W_t s_t / 2^64), W_t = x | y << 32 of Philox4x32-10 at the counter (i, j, t, 7) under the key
 *           (seed & 0xffffffff, seed >> 32); the selected member carries the multiplier s_t.  The multipliers sum to u and a
 *           member is selected with probability 1 / s_t (up to the 2^-64 s_t bias of the multiply-high).
 * A selected entry has (wa, wb) = the entry weights of ocn_cn_gather, then wa' = wa * (float)s and wb' = wb * (float)s, each
 * rounded once; h[k] is fetched exactly when wa' != 0 or wb' != 0 and then added to both sums, one rounded multiply and one
 * add per feature, in ascending position: ocn_cn_gather's order, arithmetic and fetch rule.  x * 1.0f is exact, so every
 * candidate with u <= cap gets, bit for bit, ocn_cn_gather's three rows.  The sample is fixed by (seed, i, j, the
 * candidate's flags): not by the batch, its order, `rec`, `perm` or the launch geometry.  xij, the skip and the store rules
 * (cnt1 / cnt2 / rec has-bits / out_row) are ocn_cn_gather_h16's, with the counts of the FULL set: a candidate whose sample
 * holds no cn1 entry gets a zero xcn1 row where one is stored at all.  With `perm`, the group costs are upper bounds.
 * mult (or NULL): int32, one word per flag position.  Every position of [off[e], off[e] + len N(src[e])) of every batch
 * row is written, unwalked candidates included: s for a selected member, 0 for any other position; nothing else — nothing
 * at or beyond flags_cap where the flag buffer holds the batch (the positions written are the flag positions read).
 * One form for every row length (a candidate whose source row is longer than `cap` is counted first: one pass over its
 * flag bytes); max_row_len is accepted and not used.  No atomics, no workspace, no LDS, no host synchronisation.
 * H in {16, 32, 64, 128, 256, 512}.  cap < 1, B < 0, another H, a NULL required pointer (rowptrA, colA, src, dst, off, flags,
 * weights, h, the outputs): OCN_EINVAL before any HIP call.  B == 0 returns 0. */
int ocn_cn_gather_cap(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                      const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flags, const int32_t* wc,
                      const float* weights /* [N][4] */, const float* h, int32_t H, int64_t max_row_len, float* xcn1,
                      float* xcn2, float* xij, const int64_t* out_row, const int32_t* cnt1, const int32_t* cnt2,
                      const uint64_t* rec /* or NULL */, const int32_t* perm /* or NULL */, int32_t cap, uint64_t seed,
                      int32_t* mult /* [flags_cap] or NULL */, void* stream);
/* The pooling from an INT8 embedding table, exact or capped.  q8 holds N rows of `row_stride` bytes, the first H of each the
 * row's int8 elements (what follows is padding and is never read); scale is fp32 [N], one per row — the image of
 * ocn_mips_topm_i8's keys, so one resident table can serve retrieval and scoring.  Every other argument up to `perm` means
 * what it means for ocn_cn_gather_h16, and (cap, seed, mult) what they mean for ocn_cn_gather_cap.  Arithmetic: element c of
 * row k is v = fl32((float)q8[k][c] * scale[k]) — the conversion is exact, the product is ONE IEEE fp32 multiply, rounded to
 * nearest even, a subnormal result kept — and from there the term is ocn_cn_gather's: one separately rounded multiply by the
 * entry weight and one add, in ascending position, strictly sequential for every row length; xij = v_i (.) v_j.  The scale
 * is never folded into an entry weight (that would move a rounding).  Hence, with D[k][c] = fl32((float)q8[k][c] * scale[k])
 * as an fp32 [N][H] table:
 *   cap == 0: xcn1, xcn2 and xij are bit for bit what ocn_cn_gather leaves for D (mult must be NULL);
 *   cap >= 1: the sample is ocn_cn_gather_cap's, unchanged — strata, Philox counter (i, j, t, 7) and key, multipliers — and
 *             xcn1, xcn2, xij and mult (every position written, unwalked candidates included) are bit for bit what
 *             ocn_cn_gather_cap leaves for D.
 * The skip and store rules (cnt1 / cnt2 / rec has-bits / out_row) are ocn_cn_gather_h16's; there is no `rowsum`.  One form
 * for every row length; max_row_len is accepted and not used.  No atomics, no workspace, no LDS, no host synchronisation: the
 * launch can be captured.  H in {16, 32, 64, 128, 256, 512}; row_stride >= H and a multiple of 16; q8 16-byte aligned.
 * B < 0, cap < 0, cap == 0 with a mult, another H, a bad row_stride: OCN_EINVAL; B == 0 then returns 0; a NULL required pointer
 * (rowptrA, colA, src, dst, off, flags, weights, q8, scale, the outputs): OCN_EINVAL — all before any HIP call. */
int ocn_cn_gather_q8(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                     const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flags, const int32_t* wc,
                     const float* weights /* [N][4] */, const int8_t* q8 /* [N] rows of row_stride bytes */,
                     int64_t row_stride, const float* scale /* [N] */, int32_t H, int64_t max_row_len, float* xcn1,
                     float* xcn2, float* xij, const int64_t* out_row, const int32_t* cnt1, const int32_t* cnt2,
                     const uint64_t* rec /* or NULL */, const int32_t* perm /* or NULL */, int32_t cap /* 0 = uncapped */,
                     uint64_t seed, int32_t* mult /* [flags_cap] or NULL */, void* stream);
/* cn8 (CNLinkPredictorbaselearnablation, model.py:3233-3449; pattern route): intersection and pooling in ONE pass.  cn8
 * pools without column weights, so a candidate's vectors depend on nothing but the candidate:
 *   xcn1[e] = sum_{k in N(i) ∩ T1(j)} h[k]   xcn2[e] = sum_{k in N(i) ∩ T2(j)} h[k]   xij[e] = h[i] (.) h[j]
 * for e = (i, j) = (src[e], dst[e]).  N(i) (row i of A) is walked in ascending column order by one lane group, hub rows
 * included, and every member's row is added at once: one fp32 add per feature and entry, in that order — the order of a
 * sequential spmm over the sorted row.  cnt1[e] / cnt2[e] = the number of members (int32).  A candidate without members
 * gets zero rows and zero counts.  No flag bytes, no histogram and no weights are written or read.
 * T1 / T2: dense bit rows (row j at bitmap + j * stride words, bit k = column k, stride * 32 >= n_cols) where given, else
 * the CSR row j (sorted columns); at least one form of each is required.  order: as for ocn_cn_flags (or NULL).
 * h is [n_cols][H] row-major fp32, H in {16, 32, 64, 128, 256, 512}; outputs [B][H], indexed by the batch row.
 * NULL pointers, B < 0, another H, a matrix with neither form or bit rows too short: OCN_EINVAL before any HIP call. */
int ocn_cn8_pool(const int64_t* rowptrA, const int32_t* colA,
                 const int64_t* rowptrT1 /* or NULL */, const int32_t* colT1 /* or NULL */,
                 const int64_t* rowptrT2 /* or NULL */, const int32_t* colT2 /* or NULL */,
                 const uint32_t* bitmapT1 /* or NULL */, int64_t bm1_stride_words,
                 const uint32_t* bitmapT2 /* or NULL */, int64_t bm2_stride_words,
                 const int64_t* src, const int64_t* dst, const int64_t* order /* or NULL */, int64_t B, int64_t n_cols,
                 const float* h, int32_t H, float* xcn1, float* xcn2, float* xij,
                 int32_t* cnt1, int32_t* cnt2, void* stream);
/* cn5 / cn7 with FROZEN column weights (ocn_amd/frozen.py; pattern route): intersection and weighted pooling in ONE pass,
 * the shape of ocn_cn8_pool with a weight row per member.  weights is a [n_cols][4] table {w1, t, inv2, 0} (row-major fp32,
 * 16-byte aligned) that ocn_cn_weights_cn5 / _cn7 formed for a REFERENCE batch and the caller kept; every candidate
 * e = (i, j) = (src[e], dst[e]) is pooled with it instead of the weights of its own batch, so nothing of a candidate depends
 * on the rest of the batch.  Per member k of N(i), with [cn1] = k in T1(j), [cn2] = k in T2(j):
 *   wa = [cn1] * weights[k][0]      wb = ([cn2] - [cn1] * weights[k][1]) * weights[k][2]
 *   xcn1[e] += wa * h[k]   xcn2[e] += wb * h[k]   exactly when wa != 0 or wb != 0 (then to both);   xij[e] = h[i] (.) h[j]
 * every difference, product and sum rounded separately, N(i) walked in ascending column order by one lane group, hub rows
 * included: bit for bit what ocn_cn_flags -> ocn_cn_gather(weights) leave for that candidate.  cnt1[e] / cnt2[e] = the
 * number of members of N(i) ∩ T1(j) / N(i) ∩ T2(j) (int32), whatever their weights.  A candidate without members gets zero
 * rows and zero counts.  No atomics, no workspace, nothing else written.
 * T1 / T2, order, h, H and the outputs: as for ocn_cn8_pool.  NULL pointers, B < 0, n_cols < 0, another H, a misaligned
 * table, a matrix with neither form or bit rows narrower than n_cols: OCN_EINVAL before any HIP call.  B == 0 returns 0. */
int ocn_cn_pool_frozen(const int64_t* rowptrA, const int32_t* colA,
                       const int64_t* rowptrT1 /* or NULL */, const int32_t* colT1 /* or NULL */,
                       const int64_t* rowptrT2 /* or NULL */, const int32_t* colT2 /* or NULL */,
                       const uint32_t* bitmapT1 /* or NULL */, int64_t bm1_stride_words,
                       const uint32_t* bitmapT2 /* or NULL */, int64_t bm2_stride_words,
                       const int64_t* src, const int64_t* dst, const int64_t* order /* or NULL */, int64_t B, int64_t n_cols,
                       const float* weights /* [n_cols][4] */, const float* h, int32_t H,
                       float* xcn1, float* xcn2, float* xij, int32_t* cnt1, int32_t* cnt2, void* stream);
/* Per-common-neighbour attribution (ocn_amd/explain.py): the sampled dense-dense product on the CN pattern of a batch whose
 * intersection pass has run.  off [B + 1], flags, wc (or NULL: pattern route) and flags_cap are that pass's; weights is the
 * [n_cols][4] table {w1, t, inv2, 0} the batch is pooled with (its own, a frozen one, cn8's unit table); g1 / g2 [B][H] are
 * the gradients of a score with respect to xcn1[e] / xcn2[e].  For candidate e, position p of row src[e] of A
 * (off[e + 1] - off[e] = the length of that row) and q = off[e] + p:
 *   k = colA[rowptrA[src[e]] + p]   f = flags[q]   c = wc ? (float)wc[q] : 1   (wa, wb) = the entry weights ocn_cn_gather
 *   pools that entry with:  wa = [f & 1] * weights[k][0]   wb = ([f & 2] * c - [f & 1] * weights[k][1]) * weights[k][2]
 *   f == 0 (no member):  attr[q] = {+0, +0}, rank[q] = -inf
 *   else, all in fp32:   d1 = sum_f h[k][f] * g1[e][f]   d2 = sum_f h[k][f] * g2[e][f]
 *                        attr[q] = {wa != 0 ? wa * d1 : +0, wb != 0 ? wb * d2 : +0}   rank[q] = attr[q][0] + attr[q][1]
 * so that sum_q attr[q][0] = <g1[e], xcn1[e]> and sum_q attr[q][1] = <g2[e], xcn2[e]> up to rounding.  h[k] is read exactly
 * when wa != 0 or wb != 0 (the pooling's fetch rule).  Every position of [off[e], off[e + 1]) of every batch row is written,
 * nothing at or beyond flags_cap, nothing in [off[B], flags_cap).  The order of the additions of a dot product depends on H
 * only — not on the launch geometry, on `order` (an optional processing order, a permutation of the batch rows) or on the
 * rest of the batch: the output is fixed by the input.  No atomics, no workspace, no LDS.
 * H in {16, 32, 64, 128, 256, 512}; weights, h, g1, g2 16-byte aligned, attr 8-byte aligned.  NULL required pointers, B < 0,
 * flags_cap < 0, another H or a misaligned pointer: OCN_EINVAL before any HIP call.  B == 0 returns 0 without a launch. */
int ocn_cn_attribution(const int64_t* rowptrA, const int32_t* colA, const int64_t* src,
                       const int64_t* order /* or NULL */, int64_t B,
                       const int64_t* off /* [B + 1] */, const uint8_t* flags, const int32_t* wc /* or NULL */,
                       int64_t flags_cap, const float* weights /* [n_cols][4] */,
                       const float* h /* [n_cols][H] */, int32_t H,
                       const float* g1 /* [B][H] */, const float* g2 /* [B][H] */,
                       float* attr /* [flags_cap][2] */, float* rank /* [flags_cap] */, void* stream);
/* Link heuristics (common neighbours, Adamic-Adar, resource allocation, Jaccard, preferential attachment and their 2-hop
 * forms: ocn_amd/heuristics.py) in ONE pass, the shape of ocn_cn8_pool with a 16-byte node row in place of an embedding row:
 *   sum1[e][q] = sum_{k in N(i) ∩ T1(j)} w[k][q]   sum2[e][q] = sum_{k in N(i) ∩ T2(j)} w[k][q]   q = 0..3
 * for e = (i, j) = (src[e], dst[e]); cnt1[e] / cnt2[e] = the number of members (int32); deg[e] (or NULL; needs rowptrT1)
 * = {length of row i of A, length of row j of T1} as fp32.  N(i) is walked in ascending column order by one lane group, hub
 * rows included: every sum starts from 0 and takes one fp32 add per member and weight column, in that order.  A candidate
 * without members gets zeros.  No atomics, no workspace; nothing of a candidate depends on the rest of the batch.
 * T1 / T2, order: as for ocn_cn8_pool, except that ALL of T2 may be NULL: then sum2 and cnt2 are written as zeros.
 * w is [n_cols][4] row-major fp32 (16-byte aligned); sum1 / sum2 [B][4], deg [B][2], all indexed by the batch row.
 * NULL required pointers, B < 0, n_cols < 0, T1 with neither form, T2 with half a CSR, bit rows narrower than n_cols,
 * deg without rowptrT1: OCN_EINVAL before any HIP call.  B == 0 returns 0. */
int ocn_cn_node_sums(const int64_t* rowptrA, const int32_t* colA,
                     const int64_t* rowptrT1 /* or NULL */, const int32_t* colT1 /* or NULL */,
                     const int64_t* rowptrT2 /* or NULL */, const int32_t* colT2 /* or NULL */,
                     const uint32_t* bitmapT1 /* or NULL */, int64_t bm1_stride_words,
                     const uint32_t* bitmapT2 /* or NULL */, int64_t bm2_stride_words,
                     const int64_t* src, const int64_t* dst, const int64_t* order /* or NULL */, int64_t B, int64_t n_cols,
                     const float* w /* [n_cols][4] */, float* sum1, float* sum2, int32_t* cnt1, int32_t* cnt2,
                     float* deg /* or NULL */, void* stream);

/* Candidate generation for link recommendation (ocn_amd/recommend.py): the row difference of two CSR matrices with the same
 * rows, for the rows a caller names.  For query q with s = rows[q] (int64; a source may repeat, its rows may be empty) the
 * set is P[s,:] \ M[s,:], without column s too when drop_self != 0, in ascending column order.  With P = the pattern of A²
 * and M = A that is the 2-hop neighbourhood of s that is not yet linked: the targets with a non-empty cn1.  (cn2 = N(s) ∩
 * pattern(A² row t) is non-empty for every target within THREE hops: those come from ocn_frontier_*, below.)
 * Two phases around a caller-side allocation, as for the A*A pattern: count -> ocn_scan_i32 -> fill.
 *   count[q] (int32) = the size of query q's set;
 *   edges (int64 [T][2], T = off[Q], 16-byte aligned) takes the pairs (s, c) of query q row-major from edges[off[q]] on: the
 *   layout of split_edge[...]['edge'], what the scoring loops take.  A pair that would land at off[q + 1] or beyond is
 *   dropped: offsets that do not belong to these inputs leave holes, they never write past their own segment.
 * Both passes run ONE kernel body: a wave owns a query, stages the M row in LDS when it has at most
 * ocn_row_diff_stage_cols() columns (searched in memory beyond), streams the P row 64 columns at a time — hub rows of A²
 * included, they only take more rounds — and compacts by ballot and popcount behind a running base.  No atomics, no
 * workspace.  Both matrices: sorted, duplicate-free int32 columns; rows[] must be valid row ids of both (not checked here).
 * NULL pointers or Q < 0: OCN_EINVAL before any HIP call.  Q == 0 returns 0. */
int32_t ocn_row_diff_stage_cols(void);
int ocn_row_diff_count(const int64_t* rowptrP, const int32_t* colP, const int64_t* rowptrM, const int32_t* colM,
                       const int64_t* rows, int64_t Q, int32_t drop_self, int32_t* count /* [Q] */, void* stream);
int ocn_row_diff_fill(const int64_t* rowptrP, const int32_t* colP, const int64_t* rowptrM, const int32_t* colM,
                      const int64_t* rows, int64_t Q, int32_t drop_self, const int64_t* off /* [Q + 1], from ocn_scan_i32 */,
                      int64_t* edges /* [off[Q]][2] */, void* stream);
/* The same candidate set without a stored A²: for query q with s = rows[q] the set is
 *   ( U_{m in A[s,:]} A[m,:] ) \ M[s,:], without column s too when drop_self != 0,
 * in ascending column order — with M = A exactly pattern(A² row s) \ (N(s) U {s}), what ocn_row_diff_* yields from a
 * materialised A².  The contract of ocn_row_diff_* holds word for word: count -> ocn_scan_i32 -> fill, count[q] int32, edges
 * int64 [off[Q]][2] pairs (s, c) row-major, a source may repeat and its rows may be empty, a pair that would land at
 * off[q + 1] or beyond is dropped.  Both passes run ONE kernel body: a workgroup owns a query and keeps the set as a bitmap in
 * LDS, as the A*A pattern kernel keeps an output row; the column limit of that kernel is lifted by sweeping the column range
 * in windows of window_cols columns (every neighbour's row is entered at the window's lower bound by binary search), so any
 * n_cols < 2^31 is served.  LDS atomics only: no global atomics, no workspace, the output is fixed by the input.
 * window_cols: 0 = ocn_two_hop_window_cols() (what fits the CU's LDS; a multiple of 64), else a positive multiple of 64 no
 * larger than that — a small window exercises the sweep on a small graph, it is never faster.  The bitmap takes
 * min(window_cols, n_cols rounded up to 64) / 8 bytes of LDS.  A and M: square, n_cols rows and columns, sorted duplicate-free
 * int32 columns; rows[] must be valid row ids (not checked here).
 * NULL pointers, Q < 0, n_cols <= 0 or >= 2^31, a bad window_cols: OCN_EINVAL before any HIP call.  Q == 0 returns 0. */
int64_t ocn_two_hop_window_cols(void);
int ocn_two_hop_diff_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                           int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self,
                           int64_t window_cols /* 0: the default */, int32_t* count /* [Q] */, void* stream);
int ocn_two_hop_diff_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                          int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self,
                          int64_t window_cols /* 0: the default */, const int64_t* off /* [Q + 1], from ocn_scan_i32 */,
                          int64_t* edges /* [off[Q]][2] */, void* stream);
/* The candidates of ocn_two_hop_diff_fill, each with a path sum (retrieve-then-rank recommendation: the cheap score the
 * candidates are short-listed by, from the expansion that enumerates them — no intersection per candidate, no A²).
 *   edges: exactly the pairs ocn_two_hop_diff_fill writes for the same arguments — the same set, the same ascending order, the
 *   same `off` protocol (off = ocn_scan_i32 of ocn_two_hop_diff_count: there is no second counting pass), a pair at off[q + 1]
 *   or beyond is dropped, and so is its value.
 *   val[p] (fp32 [off[Q]]) for the pair (s, c) at position p = the sum of w[m][wcol] over the m in row s of A whose row holds c,
 *   taken in ASCENDING m, one fp32 add per member, starting from 0.0f, plain adds without contraction.  w: a node table
 *   [n_cols][4] row-major (the table of ocn_cn_node_sums), wcol its column 0 .. 3; w == NULL: every weight is 1.0f and wcol is
 *   ignored.  For a symmetric A that is, bit for bit, what ocn_cn_node_sums adds up for the candidate (s, c) over
 *   N(s) ∩ N(c): w == NULL the common-neighbour count, the columns of 1 / log deg and 1 / deg Adamic-Adar and resource allocation.
 *   Membership is a presence bit, not val != 0: a candidate whose sum is zero or negative is emitted like any other.
 * A workgroup owns a query; a window keeps one presence bit and one fp32 accumulator per column in LDS, so it is
 * ocn_two_hop_sums_window_cols() columns wide (about 39 000, a multiple of 64) and any n_cols < 2^31 is swept in such windows.
 * Each of the four waves owns a contiguous quarter of the window's columns and walks all neighbours of s in ascending order,
 * so an accumulator is touched by one wave only, in program order: LDS atomics on the presence bits alone, no float atomics,
 * no global atomics, no workspace — val is fixed by the input.  window_cols: 0 = the default, else a positive multiple of 64
 * no larger than it (for tests of the sweep on small graphs).  The launch has at most 4 096 workgroups; beyond that many
 * queries a workgroup takes several, grid-stride.  LDS: min(window_cols, n_cols rounded up to 64) * 33 / 8 bytes.
 * A and M as for ocn_two_hop_diff_*; rows[] must be valid row ids (not checked here).
 * NULL rowptrA / colA / rowptrM / colM / rows / off / edges / val, Q < 0, n_cols <= 0 or >= 2^31, a bad window_cols, wcol
 * outside 0 .. 3 with w given: OCN_EINVAL before any HIP call.  Q == 0 returns 0. */
int64_t ocn_two_hop_sums_window_cols(void);
int ocn_two_hop_sums_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                          int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self,
                          int64_t window_cols /* 0: the default */,
                          const float* w /* [n_cols][4] row-major, or NULL: every weight 1.0f */,
                          int32_t wcol /* 0 .. 3, ignored when w == NULL */, const int64_t* off /* [Q + 1] */,
                          int64_t* edges /* [off[Q]][2] */, float* val /* [off[Q]] */, void* stream);
/* Frontier expansion with ordered path sums: ocn_two_hop_sums_fill with the frontier made explicit, so that expansions chain —
 * the output of one is the frontier (and the seed) of the next, one hop per launch.  For query q with s = rows[q]:
 *   the frontier F_q: the entries ptrF[q] .. ptrF[q + 1] of a pair list — node c = nodeF[2 i + 1] (the second word of pair i: the
 *   int64 [T][2] layout the fills of this family write, its first word is not read), weight f_c = valF[i] (fp32; valF == NULL:
 *   every weight is 1.0f) — ascending in c and duplicate-free;
 *   the seeds S_q (ptrS == nodeS == NULL: none): the same layout, node t and value v_t = valS[i], ascending and duplicate-free.
 * The set is ( U_{c in F_q} A[c,:]  U  nodes(S_q) ) \ M[s,:], without column s too when drop_self != 0, in ascending column
 * order; val of the pair (s, t) = v_t where t is seeded, else 0.0f, plus f_c for every c in F_q whose row holds t, the adds in
 * ASCENDING c, one fp32 add per member, plain adds without contraction.  Membership is the presence bit, never val != 0.
 * With F_q = the row of s in A weighted by a node table and no seeds that is ocn_two_hop_diff_count / ocn_two_hop_sums_fill,
 * bit for bit.  With F = the unexcluded 2-hop expansion L2 of s, f_c = decay * w[c] * P2(s, c), the seeds (L2, P2) and M = the
 * known links, val = P2 + decay * P3: the candidates within three hops — every target with a non-empty cn1 or cn2 — and
 * their local path index.
 * The protocol is that of ocn_two_hop_diff_* / ocn_two_hop_sums_fill word for word: count -> ocn_scan_i32 -> fill, count[q]
 * int32, edges int64 [off[Q]][2] pairs (s, t) row-major, a pair that would land at off[q + 1] or beyond is dropped, and so is
 * its value; a source may repeat, a list may be empty, a frontier node may have an empty row.  ocn_frontier_sums_fill with
 * val == NULL writes the pairs alone (valF and valS are then not read).
 * One kernel body for the three passes.  A workgroup owns a query; a window keeps one presence bit and (with values) one fp32
 * accumulator per column in LDS, ocn_frontier_window_cols() columns (38 208, a multiple of 64), and any n_cols < 2^31 is swept
 * in such windows.  Each of the four waves owns a contiguous quarter of the window's columns, enters the seeds of its quarter
 * and then walks the whole frontier in ascending order, 64 entries at a time: entries with one column in the quarter add side
 * by side — lanes that meet in a column take turns in lane order through a claim table in LDS — entries with several are walked
 * by the wave.  An accumulator is touched by one wave only, in program order: LDS atomics on the presence bits and the claim
 * table alone, no float atomics, no global atomics, no workspace — the output is fixed by the input.
 * window_cols: 0 = the default, else a positive multiple of 64 no larger than it (for tests of the sweep on small graphs).
 * The launch has at most 4 096 workgroups; beyond that many queries a workgroup takes several, grid-stride.
 * LDS: min(window_cols, n_cols rounded up to 64) / 8 bytes, * 33 / 8 with values, and 4 KiB of claim tables with values.
 * A and M: square, n_cols rows and columns, sorted duplicate-free int32 columns.  rows[] and the nodes of both lists must be
 * valid row ids, the lists sorted (not checked here).
 * NULL rowptrA / colA / rowptrM / colM / rows / ptrF / nodeF / count resp. off / edges, ptrS without nodeS or the reverse, seeds
 * without valS where val is written, Q < 0, n_cols <= 0 or >= 2^31, a bad window_cols: OCN_EINVAL before any HIP call.
 * Q == 0 returns 0. */
int64_t ocn_frontier_window_cols(void);
int ocn_frontier_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                       const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols /* 0: the default */,
                       const int64_t* ptrF /* [Q + 1] */, const int64_t* nodeF /* [ptrF[Q]][2] */,
                       const int64_t* ptrS /* [Q + 1] or NULL */, const int64_t* nodeS /* [ptrS[Q]][2] or NULL */,
                       int32_t* count /* [Q] */, void* stream);
int ocn_frontier_sums_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                           int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self,
                           int64_t window_cols /* 0: the default */, const int64_t* ptrF /* [Q + 1] */,
                           const int64_t* nodeF /* [ptrF[Q]][2] */, const float* valF /* [ptrF[Q]] or NULL: every weight 1.0f */,
                           const int64_t* ptrS /* [Q + 1] or NULL */, const int64_t* nodeS /* [ptrS[Q]][2] or NULL */,
                           const float* valS /* [ptrS[Q]] */, const int64_t* off /* [Q + 1], from ocn_scan_i32 */,
                           int64_t* edges /* [off[Q]][2] */, float* val /* [off[Q]] or NULL: not written */, void* stream);
/* The k best entries of every segment scores[ptr[q] .. ptr[q + 1]) of a flat fp32 vector, best first, 1 <= k <=
 * ocn_segment_topk_max_k() (128: two slots per lane).  top_val [Q][k] = the scores, top_pos [Q][k] (int64) = their positions
 * in the FLAT vector, so that one index gathers whatever else the caller keeps per entry; a segment with fewer than k
 * entries fills the rest with -inf and -1.  The order is total and part of the contract: the higher score first (fp32
 * comparison, +0.0 == -0.0); equal scores by ascending position; NaN after every number, -inf included, NaNs among
 * themselves by position.  The scores are returned as they were stored (a NaN's payload and a zero's sign survive).
 * A wave owns a segment and keeps its running best sorted across its lanes; the segment is consumed 64 scores at a time
 * and a chunk in which nothing beats the current k-th best costs one ballot.  Segments are independent: no atomics, no
 * workspace, the result is fixed by the input.  A segment must have fewer than 2^32 - 1 entries.
 * NULL pointers, Q < 0, k < 1 or k above the limit: OCN_EINVAL before any HIP call.  Q == 0 returns 0. */
int32_t ocn_segment_topk_max_k(void);
int ocn_segment_topk(const float* scores, const int64_t* ptr, int64_t Q, int32_t k, float* top_val, int64_t* top_pos,
                     void* stream);
/* The place of given nodes in that order: a segmented rank.  Segment q is scores[ptr[q] .. ptr[q + 1]) and its ids are
 * edges[.][1] over the same range — the [T][2] pair layout every candidate builder writes — ASCENDING within a segment
 * (trusted, not checked, as ptr is).  tnode[tptr[q] .. tptr[q + 1]) are the nodes to rank in segment q: in any order, with
 * repeats, possibly none; tptr [Q + 1] ascends from 0 to P.  For target j of segment q: rank[j] = 0 and pos[j] = -1 where
 * tnode[j] is no id of the segment (any int64 value: negative and out-of-range ids simply are not found); else pos[j] is the
 * entry's position in the FLAT vector and rank[j] = 1 + the number of entries of the segment that precede it in the total
 * order of ocn_segment_topk — the 1-based place it takes in an unbounded top-k, so rank <= k exactly when ocn_segment_topk(k)
 * lists it, at top_pos[q][rank - 1].
 * A wave owns a target: it finds its segment by a search of its own index in tptr (no work list), the node by a binary
 * search of the ids, and streams the segment's scores counting the keys that beat the target's.  No sort, no atomics, no
 * workspace, no barriers; the result is fixed by the input.  A segment must have fewer than 2^32 - 1 entries.
 * NULL pointers, Q < 0, P < 0: OCN_EINVAL before any HIP call.  Q == 0 or P == 0 returns 0 and launches nothing. */
int ocn_segment_rank(const float* scores, const int64_t* ptr, const int64_t* edges /* [ptr[Q]][2] */, int64_t Q,
                     const int64_t* tptr /* [Q + 1] */, const int64_t* tnode /* [P] */, int64_t P,
                     int64_t* rank /* [P] */, int64_t* pos /* [P] */, void* stream);
/* The m best entries of every segment in that order, as a SET: what a short list needs, for any 1 <= m <= 2^31 - 1 (no
 * limit of ocn_segment_topk applies).  ptr_m [Q + 1] is formed by the caller as the scan of min(ptr[q + 1] - ptr[q], m); the
 * positions in the FLAT vector of the min(len, m) entries of segment q that come first in the total order of
 * ocn_segment_topk are written to keep_pos[ptr_m[q] .. ptr_m[q + 1]), ASCENDING — within a segment of a candidate list that
 * is ascending node id.  Keys are distinct, so exactly min(len, m) entries are kept and they are ocn_segment_topk's where
 * m is within its limit.  cut (may be NULL) [Q]: the key of the worst kept entry of segment q — high word the score's
 * monotone image (-0.0 folded onto +0.0, NaN = 0), low word ~(position in the segment) — 0 for an empty segment.
 * A workgroup owns a segment.  len <= m: copied through.  Else the m-th best image is found by an MSB-first radix select,
 * four passes of 8 bits over a 256-bin histogram in LDS (integer LDS atomics: the counts do not depend on their order), and
 * one ordered compaction pass keeps what lies above the cut image U and the first r entries that equal it.  No float
 * atomics, no global atomics, no workspace; the result is fixed by the segment alone.  The segment is read five times (the
 * later passes from L2 at the sizes a 2-hop or 3-hop list has), and the longest segment sets the launch's tail, as it does
 * for ocn_segment_topk and ocn_segment_rank.  Whatever scores holds, nothing is written outside [ptr_m[q], ptr_m[q + 1]).
 * A segment must have fewer than 2^32 - 1 entries.
 * NULL pointers (cut excepted), Q < 0, m < 1 or m > 2^31 - 1: OCN_EINVAL before any HIP call.  Q == 0 returns 0. */
int ocn_segment_keep_best(const float* scores, const int64_t* ptr, int64_t Q, int64_t m, const int64_t* ptr_m /* [Q + 1] */,
                          int64_t* keep_pos /* [ptr_m[Q]] */, uint64_t* cut /* [Q] or NULL */, void* stream);

/* Structured negative sampling (ocn_amd/sampling.py): pairs that are guaranteed not to be links of a square `known` matrix
 * (sorted, duplicate-free int32 columns, n_cols rows and columns, 1 <= n_cols < 2^31), drawn exactly uniformly, with
 * replacement, without a rejection loop — a hub row or a dense graph costs what a sparse one does.  Where the reference
 * calls PyG's negative_sampling (NeighborOverlap_large.py:51, NeighborOverlap_large_ppa.py:67) these entries draw on the device from the CSR the
 * scoring loops read.
 *
 * For a row s the excluded set is X(s) = known[s,:] U {s} — s is counted once, whether or not the row stores it — and its
 * complement C(s) has m_s = n_cols - |X(s)| members.  The r-th smallest member of C(s) (0-based) is r + i, where i is the
 * smallest index with x_i - i > r over the ascending members x_0 < x_1 < ... of X(s), and |X(s)| if there is none: a binary
 * search on the row.
 *
 * Random words: Philox4x32-10 with the Random123 constants (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 * 0xBB67AE85; ten rounds), key = (seed & 0xffffffff, seed >> 32).  A draw takes u = out[0] | out[1] << 32 of one counter and
 * r = floor(u * m / 2^64) (the high word of the 128-bit product: a bias below m / 2^64).  Counters:
 *   per-source sample j of query q : (j, q & 0xffffffff, q >> 32, 2)
 *   pair sample t                  : (t & 0xffffffff, t >> 32, 0, 1)
 * so a sample is a function of (seed, its own index, known) and of nothing else — not of the launch geometry, not of per, Q
 * or T.  No atomics, no workspace, the output is fixed by the input.
 *
 * ocn_philox4x32: out[i] = Philox4x32-10(ctr[i], (key0, key1)), the generator itself; ctr and out 16-byte aligned.
 * ocn_complement_count: count[s] = m_s for every row; ocn_scan_i32 of it gives the int64 prefix cptr[n_cols + 1], whose last
 *   entry is M, the number of ordered non-edge, non-self pairs.
 * ocn_sample_complement_rows: out[q][j] (int64 [Q][per], 1 <= per < 2^31) = the member of C(rows[q]) selected by the counter
 *   of (q0 + q, j), or -1 where m_s == 0.  q0 >= 0 lets a caller produce a long split in chunks with identical results.  A
 *   wave owns one (query, 64-sample chunk): it stages the row in LDS when it has at most ocn_sample_stage_cols() columns
 *   (searched in memory beyond) and stores 64 consecutive samples.  rows[] must be valid row ids (not checked here).
 * ocn_sample_complement_pairs: sample t0 + t draws r in [0, M) with M = cptr[n_cols]; its row s is the last row with
 *   cptr[s] <= r (a row with an empty complement is never chosen), its column the member of C(s) of rank r - cptr[s]:
 *   uniform over the ordered non-edge, non-self pairs.  out (int64 [2][T]) = sources, then targets: the layout of tar_ei.
 *   One thread per sample.  M == 0 is the caller's to refuse: the kernel then writes -1 and searches nothing.
 * NULL pointers, Q / T / n < 0, q0 / t0 < 0, n_cols outside 1 .. 2^31 - 1, per outside 1 .. 2^31 - 1: OCN_EINVAL before any
 * HIP call.  Q == 0, T == 0, n == 0 return 0 (after the checks). */
int ocn_philox4x32(const uint32_t* ctr /* [n][4] */, uint32_t key0, uint32_t key1, int64_t n, uint32_t* out /* [n][4] */,
                   void* stream);
int ocn_complement_count(const int64_t* rowptrK, const int32_t* colK, int64_t n_cols, int32_t* count /* [n_cols] */,
                         void* stream);
int32_t ocn_sample_stage_cols(void);
int ocn_sample_complement_rows(const int64_t* rowptrK, const int32_t* colK, int64_t n_cols, const int64_t* rows, int64_t Q,
                               int64_t per, int64_t q0, uint64_t seed, int64_t* out /* [Q][per] */, void* stream);
int ocn_sample_complement_pairs(const int64_t* rowptrK, const int32_t* colK, int64_t n_cols,
                                const int64_t* cptr /* [n_cols + 1] */, int64_t T, int64_t t0, uint64_t seed,
                                int64_t* out /* [2][T] */, void* stream);

/* Hard negatives: draws from the candidate set that recommendation serves, not from all non-links.  For query q with
 * s = rows[q] the set H_q is that of ocn_two_hop_diff_count / _fill word for word,
 *   ( U_{m in A[s,:]} A[m,:] ) \ M[s,:], without column s too when drop_self != 0,
 * and c_q = |H_q| (written to count[q] where count is given: ocn_two_hop_diff_count's value).  Query q owns the slots
 * sptr[q] .. sptr[q + 1] of out (sptr ascends from 0 and is trusted, as `off` is elsewhere; a query may own none; a source
 * may repeat).  Slot i receives the r_i-th smallest member of H_q (0-based), r_i = floor(u_i * c_q / 2^64) for the 64-bit word
 * u_i = out[0] | out[1] << 32 of Philox4x32-10 under the key rule above, with counters of their own streams:
 *   sid == NULL : (i - sptr[q], (q0 + q) & 0xffffffff, (q0 + q) >> 32, 3)
 *   sid given   : (sid[i] & 0xffffffff, sid[i] >> 32, 0, 4), and q0 is ignored
 * — uniform over H_q with replacement — or -1 where H_q is empty.  A sample is fixed bit for bit by (seed, its own index, A,
 * M, s): not by the window width, the launch geometry, Q or the other slots.  No global atomics, no workspace.
 * The candidates are never listed: a workgroup owns a query, builds each window's part of H_q as the LDS bitmap of
 * ocn_two_hop_diff_* (the same device function), keeps the block scan of its threads' popcounts in LDS, and one thread per
 * slot finds its member there (a search of the thread prefixes, a walk of one thread's words, the n-th set bit).  Where the
 * column range fits one window the same expansion yields c_q and the selection; a wider graph is swept twice, once for c_q
 * and once selecting behind a running base.  The prefix table takes LDS from the bitmap: the default window is this entry's
 * own, ocn_sample_two_hop_window_cols() (a multiple of 64, about 1.28 M columns).  window_cols, A, M, rows[]: as for
 * ocn_two_hop_diff_*, against that limit.
 * NULL pointers (sid and count excepted), Q < 0, q0 < 0, n_cols outside 1 .. 2^31 - 1, a bad window_cols: OCN_EINVAL before any
 * HIP call.  Q == 0 returns 0 (after the checks). */
int64_t ocn_sample_two_hop_window_cols(void);
int ocn_sample_two_hop(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                       const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols /* 0: the default */,
                       const int64_t* sptr /* [Q + 1] */, const int64_t* sid /* [sptr[Q]] or NULL */, int64_t q0, uint64_t seed,
                       int32_t* count /* [Q] or NULL */, int64_t* out /* [sptr[Q]] */, void* stream);

/* Random-walk retrieval: the candidates of a source from W short uniform walks, not from its whole neighbourhood.  The visit
 * counts are a Monte-Carlo estimate of the "ra" path index that ocn_two_hop_sums_fill / ocn_frontier_sums_fill compute
 * exactly: E[c2(t)] / W = RA(s, t) / deg s and E[c3(t)] / W = P3_ra(s, t) / deg s.  The cost is
 * W * L dependent row reads per source, whatever its degree.
 *
 * A, M: CSR, sorted duplicate-free int32 columns, n_cols rows and columns (1 <= n_cols < 2^31); the walk follows the rows of A
 * as they are given (a directed A is legal), M is the exclusion.  sources[]: valid row ids (a source may repeat).
 * Walk w (0 <= w < walks) of source s starts at p_0 = s.  Step t = 1 .. length: where row p_{t-1} of A is empty the walk ends;
 * else p_t = colA[rowptrA[p_{t-1}] + floor(u_t * deg(p_{t-1}) / 2^64)].  Random words (Philox4x32-10 and the key rule of the
 * samplers above): u_1 = out[0] | out[1] << 32 and u_2 = out[2] | out[3] << 32 of the counter (w, s & 0xffffffff, s >> 32, 5),
 * u_3 = out[0] | out[1] << 32 of the counter (w, s & 0xffffffff, s >> 32, 6).  The counter carries the SOURCE id, not the query
 * index: a source's walks depend on (seed, s, A, walks, length) alone, not on the other queries or their order.
 * c2[v] = the walks with p_2 = v, c3[v] = those with p_3 = v (length 3 only); p_1 is never counted.  The candidates of s are
 * the nodes with c2 + c3 > 0 that are neither s nor in row s of M.
 *
 * ocn_rw_visits_count: count[q] = the candidates of sources[q]; ocn_scan_i32 of it gives ptr.
 * ocn_rw_visits_fill: the same walks again; from ptr[q] on, in ASCENDING node id, edges = (s, v), visits = (c2, c3) and
 *   val = (float)c2 + decay * (float)c3 — one rounded product, one rounded add; (float)c2 at length 2, where decay is not read.
 *   Nothing is written at or past ptr[q + 1].  edges 16-byte aligned, visits 8-byte aligned.
 * One workgroup per query.  The visits are counted in an open-addressing table in LDS (a compare-and-swap claims a node's slot,
 * an integer add counts), sized from walks * (length - 1) so that it cannot overflow: no status, no fallback, and the counts
 * depend on neither the schedule nor the launch geometry.  The survivors are sorted by node id in LDS.  No global atomics, no
 * workspace.  ocn_rw_max_walks(): the largest `walks` the LDS of a CU holds at length 3 (at least 1024, at most 65535: the
 * counts are 16-bit fields of one word).
 * NULL pointers, Q < 0, n_cols outside 1 .. 2^31 - 1, walks outside 1 .. ocn_rw_max_walks(), length outside {2, 3}, a decay that
 * is negative or not finite, a misaligned edges / visits: OCN_EINVAL before any HIP call.  Q == 0 returns 0 (after the checks). */
int32_t ocn_rw_max_walks(void);
int ocn_rw_visits_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                        const int64_t* sources, int64_t Q, int32_t walks, int32_t length, uint64_t seed,
                        int32_t* count /* [Q] */, void* stream);
int ocn_rw_visits_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                       const int64_t* sources, int64_t Q, int32_t walks, int32_t length, uint64_t seed,
                       const int64_t* ptr /* [Q + 1] */, float decay, int64_t* edges /* [ptr[Q]][2] */, float* val /* [ptr[Q]] */,
                       int32_t* visits /* [ptr[Q]][2] */, void* stream);

/* Embedding retrieval: for every query the m nodes with the largest inner product against it, over ALL nodes — brute force,
 * exact, without a [Q][N] score matrix.  The other retrieval stages are graph-local (a target beyond three hops is never
 * proposed, a source without neighbours gets nothing); this one reads the embeddings alone ("Embedding
 * retrieval").
 *
 * query int8 [Q][H], keys int8 [N][H] (row-major, 16-byte aligned, operands expected in [-127, 127]: -128 is not validated),
 * kscale fp32 [N].  dot[q][n] = sum_f query[q][f] * keys[n][f] in int32 on v_mfma_i32_32x32x32_i8, exact: H <= 1024, so
 * |dot| <= 1024 * 127^2 < 2^24.  val[q][n] = (float)dot[q][n] * kscale[n] — the conversion is exact, the one fp32 multiply is the
 * only rounding.  H must be a positive multiple of ocn_mips_h_align() (64) — zero padding changes no dot product.
 * Eligibility: with rows [Q] (the node id of every query, a source may repeat), node n is eligible for query q unless
 * drop_self != 0 and n == rows[q], or colM is given and n is in row rows[q] of M (CSR over the N nodes, sorted duplicate-free
 * int32 columns, as for ocn_row_diff_*; a rows[q] outside [0, N) has no row of M and excludes nothing).  Without rows every
 * node is eligible and drop_self is not read.
 * Order: the eligible nodes of a query in the total order of ocn_segment_topk with the NODE ID as the position — the higher val
 * first, +0.0 == -0.0, equal values to the lower node id, NaN (a kscale that is not finite) after every number.  top_val [Q][m] /
 * top_node [Q][m] are the first m, best first, padded with -inf / -1 where fewer than m nodes are eligible, 1 <= m <=
 * ocn_mips_max_m() (= ocn_segment_topk_max_k()).  top_val is the value as ordered: a -0.0 is returned as +0.0.
 * A wave owns 32 queries (the B operand, fragments in registers for H = 64, 128, 256) and keeps their sorted lists of m 64-bit
 * keys in LDS; the four waves of a workgroup stream the same contiguous slice of the key range, 32 keys (the A operand) at a
 * time.  An accumulator tile is converted, scaled and tested against the m-th best of its query — one compare per element where
 * nothing passes; the few that pass are checked for eligibility (a binary search in the row of M) and inserted, one round trip
 * to LDS each.  n_split slices
 * (0 = chosen from Q, N and m to fill the device; no more slices than there are 32-key tiles) leave partial lists in the
 * workspace, which a second kernel merges per query in the same order.  Keys are distinct, so the output is fixed by the inputs
 * alone: not by n_split, the grid, the tile shape or the other queries.  No float atomics, no allocation, no host sync, no
 * global state.  workspace: ocn_mips_workspace_bytes(Q, N, m, n_split) bytes (-1 for arguments the entry refuses), 8-byte
 * aligned, any content.
 * NULL query / keys / kscale / top_val / top_node / workspace, Q < 0, N outside 1 .. 2^31 - 1, H no positive multiple of
 * ocn_mips_h_align() or above 1024, m outside 1 .. ocn_mips_max_m(), n_split < 0, rowptrM without colM or the reverse, M
 * without rows, a query, keys or kscale that is not 16-byte aligned, a workspace that is not 8-byte aligned: OCN_EINVAL before
 * any HIP call.  Q == 0 returns 0 (after the checks). */
int32_t ocn_mips_max_m(void);
int32_t ocn_mips_h_align(void);
int64_t ocn_mips_workspace_bytes(int64_t Q, int64_t N, int32_t m, int32_t n_split);
int ocn_mips_topm_i8(const int8_t* query /* [Q][H] */, const int8_t* keys /* [N][H] */, const float* kscale /* [N] */,
                     int64_t Q, int64_t N, int32_t H, const int64_t* rows /* [Q] source ids, or NULL */,
                     const int64_t* rowptrM, const int32_t* colM /* exclusion CSR, or both NULL */, int32_t drop_self,
                     int32_t m, int32_t n_split /* 0 = auto */, float* top_val /* [Q][m] */, int64_t* top_node /* [Q][m] */,
                     void* workspace, void* stream);

/* The pooling's visiting order at H = 256 (a workgroup = OCN_SCHED_GROUP candidates = one group of ocn_cn_flags' gcost): candidates
 * differ 100x in cost and the few with hundreds of rows, met late, end the kernel as stragglers (0.206 -> 0.17 ms at the
 * collab shape).  perm[] = inside each XCD's contiguous eighth of the groups, the groups stable-sorted by descending cost:
 * groups of one source keep one cost and stay neighbours (L2).  n_groups = B / OCN_SCHED_GROUP, a multiple of OCN_SCHED_EIGHTHS, at most
 * OCN_SCHED_EIGHTHS * OCN_SCHED_MAX_EIGHTH (else OCN_EINVAL).
 * segment > 0 (dividing an eighth): the sort runs inside consecutive segments of that many groups instead of over the whole
 * eighth — the sources in flight on an XCD then stay within a narrow range of the source order (what their rows' L2
 * residency depends on) while every segment still starts with its longest jobs; 0 = whole eighths. */
int ocn_gather_schedule(const int32_t* gcost, int64_t n_groups, int64_t segment, int32_t* perm, void* stream);
/* H = 256 batches of at least `min_rows` candidates, fed by slot records on the pattern route without `rowsum`, are pooled with
 * TWO neighbouring slots of one group per wave (cn_pool.hip: cn_gather_pair_kernel): both slots' records, chunks of N(src), flag
 * bytes, column weights, embedding rows and endpoint rows are in flight together, and a pair of one source loads each row
 * once.  A workgroup is then two groups: `perm` is followed where an XCD's eighth holds an even number of groups (an odd one
 * keeps the one-slot form); without `perm` the pairs are consecutive groups.  Every output is bit for bit what the one-slot
 * form writes (tests/test_pool_pairs_gpu.py).  Sets the bound (process-wide; default 32768) and returns the previous one; a
 * negative argument only queries. */
int64_t ocn_cn_gather_pair_min_batch(int64_t min_rows);

/* The 3-hop predictor cn6 (model.py:2535-2951), pattern route.  Two intersection passes over the same
 * candidate batch — (A, A, A²) into flagsA / histA and (A, A³) into flagsB / histB (bit 0 = cn3 entry,
 * n1 field = cn3 column count) — then:
 *   ocn_cn_weights_cn6: histA -> {inv1, t, inv2, 0} exactly as cn5 (:2546-2714), histB -> {1/S3,0,0,0}
 *     with S3 the column sums of cn3 - nip*ncn1 - nip*ncn2' over the union pattern (:2846-2931; in
 *     eval all three inner products are the stored buffer), nip_out[0] = nip;
 *   ocn_cn_gather3: xcn1, xcn2, xcn3 = spmm_add of the three normalised matrices (:2712-2713, :2933),
 *     xij = x_i * x_j.  H in {16, 32, 64, 128, 256, 512}. */
int ocn_cn_weights_cn6(uint64_t* histA, uint64_t* histB, int64_t N, const float* innerprod, int32_t* scalars,
                       float* nip_out, const float* s2_exact /* or NULL */, const float* s3_exact /* or NULL */,
                       void* stream);
int ocn_cn_gather3(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                   const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flagsA,
                   const uint8_t* flagsB, const float* weightsA, const float* weightsB, const float* nip,
                   const float* h, int32_t H, float* xcn1, float* xcn2, float* xcn3, float* xij, void* stream);

/* The (A, A³) pass of cn6 WITHOUT a stored A³.  For e = (i, j) the p-th neighbour k of i is a cn3 entry exactly when
 * A³[j, k] != 0: when some m with A[m, k] != 0 has A²[j, m] != 0, i.e. when row k of Aᵀ shares a column with row j of A².
 * The pass walks the neighbours of the neighbours of the source and probes bit row j of A² (one probe per membership test);
 * its outputs are byte for byte what ocn_cn_flags leaves when called with T1 = the pattern of A·A·A and no T2 on the same
 * src / dst / off:
 *   flags[off[e] + p] = OCN_F_CN1 where neighbour p of src[e] is a cn3 entry, else 0 — every position of every row is written;
 *   cnt3[e] = the number of entries; hist[k] word 0 += 1 | 1 << 42 per entry of column k (n1 and n_union, what
 *   ocn_cn_weights_cn6 reads for its B histogram), word 1 is untouched.  hist and cnt3 must be ZERO on entry (entries add
 *   into them with integer atomics: the result does not depend on the schedule).
 * rowptrT / colT: the CSR of Aᵀ — row k = the m with A[m, k] != 0; pass A's own arrays for a symmetric A.
 * bitmapP: dense bit rows of the pattern of A·A (row j at bitmapP + j * bm_stride_words, bit m = column m;
 * bm_stride_words * 32 >= n_cols).  off: as ocn_edge_offsets / ocn_batch_prep leave it for (rowptrA, src).
 * chunk_off: ocn_chunk_offsets(rowptrA, nds, src, order, B) — the work items: a candidate with a run of consecutive
 * neighbours of its source, the run length adapted by nds so that an item sweeps a bounded number of elements.  nds (or NULL:
 * runs of ocn_walk_chunk() neighbours) must be the array chunk_off was formed with; nds[i] = sum over k in N(i) of the length
 * of row k of Aᵀ (ocn_neighbor_degree_sum for a symmetric A).  order: as for ocn_cn_flags, it changes the processing order only.
 * status: int32[4] as for ocn_cn_flags: OCN_ST_CAP if off[B] > flags_cap (rows that do not fit are not written: nothing past
 * the cap), OCN_ST_SCAN if off[B] or chunk_off[B] is OCN_SCAN_POISON (the batch is then treated as empty); both also ORed into
 * the sticky word status[3].  No allocation, no global state, no host synchronisation.
 * NULL required pointers, negative sizes, bit rows narrower than n_cols, B >= 2^21: OCN_EINVAL before any HIP call.  B == 0
 * returns 0. */
int ocn_cn3_flags(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT, const int32_t* colT,
                  const uint32_t* bitmapP, int64_t bm_stride_words, const int64_t* src, const int64_t* dst,
                  const int64_t* order /* or NULL */, int64_t B, int64_t n_cols, const int64_t* off, uint8_t* flags,
                  int64_t flags_cap, uint64_t* hist /* [n_cols][2] */, int32_t* cnt3, int32_t* status,
                  const int64_t* nds /* or NULL */, const int64_t* chunk_off /* [B + 1] */, void* stream);

/* Backward of the pooling with respect to h (training drop-in): for upstream
 * gradients g1, g2, g3 of xcn1, xcn2, xij ([B][H] each),
 *   dh[k] += w1[k] g1[e] + w2(e,k) g2[e]  over the CN entries (the transposed spmm_add),
 *   dh[i] += g3[e] (.) h[j],  dh[j] += g3[e] (.) h[i].
 * dh [N][H] must be initialised by the caller (zeros); fp32 atomic adds (summation order varies
 * between runs).  H in {16..512, power of two}. */
/* Backward of ocn_cn_gather3 with respect to h (cn6 under autograd, model.py:2535-2951): dh[k] += w1 g1[e] + w2 g2[e] + w3 g3[e]
 * over the union entries — the weights formed as the forward forms them —, dh[i] += g4[e] * h[j], dh[j] += g4[e] * h[i];
 * fp32 atomics into dh (zeroed by the caller). */
int ocn_cn_gather3_backward(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                            const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flagsA,
                            const uint8_t* flagsB, const float* weightsA, const float* weightsB, const float* nip,
                            const float* h, int32_t H, const float* g1, const float* g2, const float* g3,
                            const float* g4, float* dh, void* stream);

int ocn_cn_gather_backward(const int64_t* rowptrA, const int32_t* colA,
                           const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                           const int64_t* off, const uint8_t* flags, const int32_t* wc,
                           const float* weights, const float* h, int32_t H,
                           const float* g1, const float* g2, const float* g3, float* dh, void* stream);

/* The same gradient without float atomics (the default of the Python layer): the batch's terms are transposed into
 * per-node lists (count -> scan -> fill -> per-list sort by flag position; the two endpoint terms of a candidate follow)
 * and ONE wave per node adds its list in that order — the same bits on every run.  dh [N][H] is read and written (the
 * caller initialises it); H a multiple of 4, <= 512; flags_cap + 2 B < 2^31. */
int64_t ocn_cn_gather_backward_det_workspace_bytes(int64_t N, int64_t B, int64_t flags_cap);
int ocn_cn_gather_backward_det(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                               int64_t B, const int64_t* off, const uint8_t* flags, const int32_t* wc, int64_t flags_cap,
                               const float* weights, const float* h, int64_t N, int32_t H, const float* g1,
                               const float* g2, const float* g3, float* dh, void* workspace, void* stream);
/* The first half of ocn_cn_gather_backward_det alone — the per-node key lists (count, scan, fill, per-list sort) — for
 * inspection: tests check the lists against a host-side reference BEFORE the accumulate pass forms addresses from them.
 * workspace as above; afterwards col_off = int64[N + 1] at its start, keys = int32[col_off[N]] at
 * ocn_cn_gather_backward_det_keys_offset(N) bytes: a key < flags_cap is the flag position of a CN entry of that node, a key
 * flags_cap + 2 e + s is candidate e's Hadamard term at its source (s = 0) or target (s = 1). */
int64_t ocn_cn_gather_backward_det_keys_offset(int64_t N);
int ocn_cn_gather_backward_det_lists(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                                     int64_t B, const int64_t* off, const uint8_t* flags, int64_t flags_cap, int64_t N,
                                     void* workspace, void* stream);

/* CSR SpMM of the encoders: torch_sparse spmm_add/mean/max (model.py:42-55), PyG GCNConv
 * propagate (model.py:58-68), pygho/torch COO @ dense (model.py:105-113).
 *   y[r] = post[r] * reduce_k( pre[r]^a * pre[k] * x[k] )  (+ self term)
 * pre/post may be NULL (= 1).  val: per-entry values of a valued adjacency (DropAdj's 1/(1-p)
 * rescale in training, model.py:198-229) or NULL (all 1).  mode: 0 sum, 1 mean, 2 max.
 * edge_scale: 0 -> entry weight is pre[k] applied to x[k] first (PureConv: n*x then A.);
 *             1 -> entry weight is fl(pre[r]*pre[k]) (GCNConv / PureConv2: normalised A).
 * self_mode: 0 none; 1 add the row's own term after the neighbours (PureConv gcn);
 *            2 insert it at its sorted column position (GCNConv fill_diag).
 * max of a valued adjacency is max_k fl(val_rk * x[k]) (torch_sparse spmm_max); an empty row gives 0.  No caller
 * passes pre, post or self_mode with mode 2; what it computes with them is the max over the same terms the sum adds (the
 * self term included), times post[r] — and 0 for a row without a term.
 * Index spaces: x has a row per COLUMN of the operator and pre an entry per row of x — pre is indexed by column id (pre[k]).
 * post is indexed by output row.  pre[r] of the output row r is read only with edge_scale = 1 or self_mode != 0, and both need
 * r to be a column id as well: the caller passes them only for an operator with no more rows than x has (self_mode: a square
 * one).  With edge_scale = 0 and self_mode = 0 the operator may be rectangular either way and pre is never indexed by a row.
 * Order of a row's terms (tests/spmm_mirror.py is this paragraph as code): the entries in ascending column order, each term
 * fl(w * x[k]) with w = pre[k] or fl(pre[r]*pre[k]), then fl(val * w) for a valued adjacency (no pre, no val: x[k] itself),
 * added as fl(acc + term); the self term, weight pre[r] or fl(pre[r]*pre[r]) (1 without pre), stands before the first column
 * >= r under self_mode 2 (at the end where there is none; an entry with column r is replaced by it, not added too) and after
 * the last entry under self_mode 1; mean divides by the number of terms added (1 where none); post[r] multiplies last. */
int ocn_spmm_csr(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows,
                 const float* x, int32_t F, const float* pre, const float* post,
                 int32_t mode, int32_t edge_scale, int32_t self_mode,
                 float* y, void* stream);

/* ocn_spmm_csr restricted to a list of output rows (refreshing the encoder output after an edge update, ocn_amd.update):
 * rows = int64 [n_list], ascending, duplicate-free, each in [0, n_rows); y is COMPACT, [n_list][F], and row i of it holds
 * what ocn_spmm_csr writes to row rows[i] of its y, bit for bit — the two entries launch one kernel body, which differs in where
 * a lane group takes its row id from (the list instead of the launch coordinates) and in nothing else: the terms of a row are
 * added in the same (column) order.  Every other operand means what it means above: pre is indexed by the GLOBAL column id,
 * post and the self term by the GLOBAL row id rows[i]; x has a row per column of the operator.  y must not overlap x (rows are
 * gathered from x while others are written).  A listed id outside [0, n_rows) gives a zero row; nothing is indexed with it.
 * F in {16, 32, 64, 128, 256, 512}.  NULL rowptr / col / x / rows / y, n_rows < 0, n_list < 0, another F, a mode or self_mode
 * out of range: OCN_EINVAL before any launch.  n_list == 0 returns 0. */
int ocn_spmm_csr_rows(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows,
                      const float* x, int32_t F, const float* pre, const float* post,
                      int32_t mode, int32_t edge_scale, int32_t self_mode,
                      const int64_t* rows, int64_t n_list, float* y, void* stream);

/* Max aggregation under autograd (model.py:42-55 aggr "max", pygho spmm aggr "amax", model.py:101-102).
 * ocn_spmm_csr_max_arg: y[i,f] = max over row i of fl(val_ik * x[k,f]) (val NULL: x[k,f]) and arg[i,f] = the column id
 *   k of the winner, the first maximum in the row's (ascending column) order; an empty row gives y = 0, arg = -1.
 *   y, arg: [n_rows, F] fp32 / int32.  Bit-equal to ocn_spmm_csr mode 2 for inputs without NaN or ±0 ties.
 * ocn_spmm_max_backward: gx[k,f] = sum over the entries (k, i) of Aᵀ with arg[i,f] == k of valT * g[i,f] (valT NULL: 1),
 *   added in Aᵀ's row order (no atomics: bit-reproducible); rowptrT / colT / valT = the CSR of Aᵀ with n_rows rows, arg and
 *   g [rows of A, F], gx [n_rows, F] (every row written).
 * F in {16, 32, 64, 128, 256, 512}; NULL pointers, n_rows < 0 or another F: OCN_EINVAL before any launch. */
int ocn_spmm_csr_max_arg(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows,
                         const float* x, int32_t F, float* y, int32_t* arg, void* stream);
int ocn_spmm_max_backward(const int64_t* rowptrT, const int32_t* colT, const float* valT, int64_t n_rows,
                          const int32_t* arg, const float* g, int32_t F, float* gx, void* stream);

/* The sampled dense-dense product on the pattern of the operator (SDDMM): the gradient of ocn_spmm_csr's y with respect to a
 * mask on its messages, at mask = 1 — out[p] = fl(c * d) for entry p of row r with column k, where
 *   w = the entry weight exactly as the forward forms it: 1 without pre, pre[k] with edge_scale = 0, fl(pre[r]*pre[k]) with
 *       edge_scale = 1, then fl(val[p]*w) for a valued adjacency;
 *   c = w, then fl(post[r]*c) with post, then fl(c / len_r) with mode 1 (len_r = the row's entry count);
 *   d = sum_f g[r][f]*x[k][f] in fp32: every lane of the row's lane group chains fused multiply-adds over its own features
 *       (ascending), an xor butterfly adds the lanes — the order depends on F only, not on the launch geometry, the row
 *       length or the rest of the matrix, so an entry has the same bits in any operator that holds it with the same operands.
 * The self term is no entry and gets no output; under self_mode 2 an entry with k == r gets +0 (the forward replaces it by the
 * self term).  rowptr / col / val / pre / post / mode / edge_scale / self_mode are ocn_spmm_csr's; g = [n_rows][F], x = one row
 * per column, out = [nnz].  Every out[p] below rowptr[n_rows] is written and nothing else; no atomics, no workspace.  Long rows
 * are cut into fixed-size runs of entries, so a hub row is many work items.
 * OCN_EINVAL before any HIP call: F outside {16, 32, 64, 128, 256, 512}; mode 2 (max has no per-message linearisation) or out
 * of range; mode 1 together with pre, post or self_mode; self_mode out of range; NULL rowptr / col / g / x / out; g or x not
 * 16-byte aligned; n_rows < 0.  n_rows == 0 (otherwise valid) returns 0 without a launch. */
int ocn_sddmm_csr(const int64_t* rowptr, const int32_t* col, const float* val /* or NULL */, int64_t n_rows,
                  const float* g /* [n_rows][F] */, const float* x /* [n_cols][F] */, int32_t F,
                  const float* pre /* or NULL */, const float* post /* or NULL */,
                  int32_t mode /* 0 sum, 1 mean */, int32_t edge_scale, int32_t self_mode,
                  float* out /* [nnz] */, void* stream);

/* out[r] = 1/sqrt(add + deg(r)) (0 where the argument is 0): rsqrt_(1+adj.sum(-1)) of
 * model.py:51,106 (add=1) and gcn_norm's deg^-1/2 (add=1 after fill_diag); deg = row length, or the
 * row sum of `val` for a valued adjacency. */
int ocn_deg_rsqrt(const int64_t* rowptr, const float* val, int64_t n_rows, float add, float* out,
                  void* stream);

/* Pattern of A*A (NeighborOverlap_large.py:68-74,112-119: spadj @ spadj, values dropped).
 * Two phases around a caller-side allocation: count -> ocn_scan_i32 -> fill.  The count phase can
 * also leave every output row as a dense bit row (288 GB of HBM make N*N/8 bytes affordable up to a
 * few hundred thousand nodes), which ocn_cn_flags then probes instead of searching the CSR row.
 * Needs n_cols <= ocn_spgemm_max_cols().  Output columns ascending per row. */
int64_t ocn_spgemm_max_cols(void);
int ocn_spgemm_pattern_count(const int64_t* rowptrA, const int32_t* colA, int64_t n_rows,
                             const int64_t* rowptrB, const int32_t* colB, int64_t n_colsB,
                             int32_t* row_count, uint32_t* bitmap /* or NULL: [n_rows][bm_stride_words] */,
                             int64_t bm_stride_words, void* stream);
int ocn_spgemm_pattern_fill(const int64_t* rowptrA, const int32_t* colA, int64_t n_rows,
                            const int64_t* rowptrB, const int32_t* colB, int64_t n_colsB,
                            const int64_t* rowptrC, int32_t* colC, void* stream);
/* Bit rows of A*B for the rows a caller is about to probe (a training step's per-batch A², NeighborOverlap_large.py:68-74, is
 * read at the candidates' target rows only): request i names row rows[i] (int64, duplicates and out-of-range ids allowed — the
 * latter are ignored); `done` (int32 [n_rows], zero before the first call, kept by the caller between calls) marks the rows that
 * exist, a row is built by the request that turns its word from 0 to 1.  Rows never requested stay unwritten.  ocn_cn_flags
 * takes such a T2 with rowptrT2 == NULL (n_cols > 8192 only: small graphs read the row lengths too). */
/* Up to this many columns ocn_cn_flags keeps a workgroup's column histogram in LDS and reads T2's row lengths beside its bit rows
 * (so T2 must come with its row pointers there). */
int32_t ocn_cn_flags_small_graph_cols(void);
/* On larger graphs, batches of at least `min_rows` candidates run the intersection pass with TWO consecutive processing slots
 * per wave (cn_flags.hip: NS = 2): both slots' records, target rows, chunks of N(src) and probes are in flight together, so a
 * CU holds twice the slots at the same registers and LDS.  Every output is bit for bit what the one-slot form writes
 * (tests/test_flags_pairs_gpu.py).  Smaller batches and the small-graph form (LDS histogram) keep one slot per wave: half as
 * many waves must still fill the chip several times over.  Sets the bound (process-wide; default 32768) and returns the
 * previous one; a negative argument only queries. */
int64_t ocn_cn_flags_pair_min_batch(int64_t min_rows);
int ocn_spgemm_bit_rows(const int64_t* rowptrA, const int32_t* colA, int64_t n_rows, const int64_t* rowptrB, const int32_t* colB,
                        int64_t n_colsB, const int64_t* rows, int64_t n_req, int32_t* done, uint32_t* bitmap,
                        int64_t bm_stride_words, void* stream);

/* The block route of utils.block_matrix_multiply (utils.py:287-323; the drivers' --adj2byblock, ogbl-ddi): A as a dense
 * 0/1 int8 matrix (ocn_dense_from_csr: dense[r][c] and its transpose, row stride ld bytes, ld a multiple of 64 >= n, both
 * ZERO on entry), each (row block, column block) of the reference's tile loop multiplied on the integer matrix cores
 * (v_mfma_i32_32x32x32_i8; the entries are walk counts, exact in int32) and the non-zero pattern OR-ed into bit rows
 * (ocn_dense_block_mm_bits: rows [r0, r1) x columns [c0, c1), block starts multiples of 32, K = inner dimension).
 * fold != 0 writes the block at its block-LOCAL position — the reference adds SparseTensor.from_dense(block), whose
 * indices are block-local, without the block's offset (utils.py:318-321): every block then lands on the
 * top-left corner; fold == 0 places it where it belongs (the intended A^2).  ocn_bitrows_count / _fill turn bit rows
 * into CSR (columns ascending). */
int ocn_dense_from_csr(const int64_t* rowptr, const int32_t* col, int64_t n, int64_t ld, int8_t* dense, int8_t* denseT,
                       void* stream);
int ocn_dense_block_mm_bits(const int8_t* A, const int8_t* Bt, int64_t ld, int64_t K, int32_t r0, int32_t r1, int32_t c0,
                            int32_t c1, int32_t fold, uint32_t* bits, int64_t bm_stride_words, void* stream);
/* Dense bit rows of a CSR pattern ([n_rows][bm_stride_words] words, ZERO on entry): what ocn_cn_flags probes as
 * bitmapT1 on small dense graphs (ogbl-ddi: 4267 nodes, 500+ neighbours each), one load per membership test instead of a
 * binary search of the target row. */
int ocn_bitrows_from_csr(const int64_t* rowptr, const int32_t* col, int64_t n_rows, uint32_t* bits, int64_t bm_stride_words,
                         void* stream);
int ocn_bitrows_count(const uint32_t* bits, int64_t bm_stride_words, int64_t n_rows, int64_t n_cols, int32_t* row_count,
                      void* stream);
int ocn_bitrows_fill(const uint32_t* bits, int64_t bm_stride_words, int64_t n_rows, int64_t n_cols, const int64_t* rowptr,
                     int32_t* col, void* stream);

/* Edge insertion into a resident graph (the reference adds its validation edges to the adjacency under
 * use_valedges_as_input, NeighborOverlap_large.py:143-145, and leaves A² stale): A' = A U D without sorting A again, and the
 * bit rows of A² updated exactly.
 *
 * ocn_csr_union_count / ocn_csr_union_fill: C[r,:] = A[r,:] U B[r,:] for two CSR patterns of the same shape, both with
 * ascending, duplicate-free int32 columns; so is the output.  Two phases around a caller-side allocation: count (int32
 * [n_rows]) -> ocn_scan_i32 -> fill (colC from rowptrC[r] on; nothing is written past rowptrC[r + 1]).  One kernel body serves
 * both passes.  A wave owns a row: a row whose other operand is empty is a coalesced copy; else every element's place is its
 * own index plus the number of smaller elements of the other row that are not duplicates (binary searches, the shorter row
 * staged in LDS up to 512 columns; no sequential merge, no atomics, no workspace), hub rows only take more rounds.
 * NULL pointers or n_rows < 0: OCN_EINVAL before any HIP call.  n_rows == 0 returns 0. */
int ocn_csr_union_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                        int64_t n_rows, int32_t* count, void* stream);
int ocn_csr_union_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                       int64_t n_rows, const int64_t* rowptrC /* [n_rows + 1], from ocn_scan_i32 */, int32_t* colC, void* stream);
/* ocn_bitrows_insert: bits |= pattern(D·A') U pattern(A'·D) in place, for square n x n patterns — with bits = the bit rows
 * of A·A and D a subset of A' = A U D, the bit rows of A'·A' (pattern(A'A') = pattern(AA) U pattern(DA') U pattern(A'D)).
 * (rowptrA, colA) = A', (rowptrT, colT) = its transpose (the same pointers where A' is symmetric), (rowptrD, colD) = D with
 * nnzD entries, bits [n][bm_stride_words] (bm_stride_words * 32 >= n), added int32 [n], ZERO on entry: added[r] becomes the
 * number of bits of row r that this call turned on.  Per entry (u, v) of D: (a) bit k of row u for every k in A' row v,
 * (b) bit v of row r for every r in A'^T row u.  Work items are chunks of at most 256 row elements, scheduled by a scan of
 * ceil(len / 256) over both kinds: a hub row is spread over many waves.  Bits are set with 32-bit atomicOr; a bit counts as
 * new exactly when the returned word did not have it, so the counts are exact when items collide and when D overlaps A or
 * repeats itself.  workspace: ocn_bitrows_insert_workspace_bytes(nnzD) bytes, any content (16-byte aligned).
 * NULL pointers, n < 0, nnzD < 0 or >= 2^30, a stride too short: OCN_EINVAL before any HIP call.  n == 0 or nnzD == 0 returns 0. */
int64_t ocn_bitrows_insert_workspace_bytes(int64_t nnzD);
int ocn_bitrows_insert(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT, const int32_t* colT,
                       const int64_t* rowptrD, const int32_t* colD, int64_t n, int64_t nnzD, uint32_t* bits,
                       int64_t bm_stride_words, int32_t* added, void* workspace, void* stream);

/* Edge removal from a resident graph — the way back from the insertion above (the reference has no counterpart: it masks
 * its target edges out of the adjacency per training batch and forms A² of the remainder from scratch,
 * NeighborOverlap_large.py:68-74; its use_valedges_as_input, NeighborOverlap_large.py:143-145, only ever adds): A' = A \ D
 * without sorting A again, and the bit rows of A² updated exactly.
 *
 * ocn_csr_minus_count / ocn_csr_minus_fill: C[r,:] = A[r,:] \ B[r,:] for two CSR patterns of the same shape, both with
 * ascending, duplicate-free int32 columns; so is the output.  The protocol of the union: count (int32 [n_rows]) ->
 * ocn_scan_i32 -> fill (colC from rowptrC[r] on; nothing is written at or past rowptrC[r + 1]).  One kernel body serves both
 * passes.  A wave owns a row: a row whose B row is empty is a coalesced copy; else the A row is streamed 64 columns at a time
 * against the B row (staged in LDS up to 512 columns, searched in memory beyond), an element B holds too is dropped and a kept
 * one lands at its own index minus the dropped ones before it (ballot prefix plus a running count; no atomics, no workspace).
 * Entries of B that A lacks are harmless.  NULL pointers or n_rows < 0: OCN_EINVAL before any HIP call.  n_rows == 0 returns 0. */
int ocn_csr_minus_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                        int64_t n_rows, int32_t* count, void* stream);
int ocn_csr_minus_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                       int64_t n_rows, const int64_t* rowptrC /* [n_rows + 1], from ocn_scan_i32 */, int32_t* colC, void* stream);
/* ocn_bitrows_remove: bits = the bit rows of A·A on entry, of A'·A' on return, in place, for square n x n patterns with
 * A' = A \ D.  A pattern cannot be decremented (that would take walk counts), but a bit can be decided again: bit (r, k) of
 * A'·A' is set exactly when row r of A' and row k of A'^T share a column, and the only bits that can differ from A·A are those
 * with a witness walk through a removed entry.  (rowptrA0, colA0) = the OLD A and (rowptrT0, colT0) its transpose: per entry
 * (u, v) of D they enumerate the candidates, (a) bit k of row u for every k in A row v, (b) bit v of row r for every r in
 * A^T row u.  (rowptrA, colA) = A' and (rowptrT, colT) its transpose decide them (where the matrices are symmetric the
 * transposes are the same pointers).  (rowptrD, colD) = D with nnzD entries; any superset of the removed entries gives the
 * same result, so D may repeat itself or name entries A never had.  bits [n][bm_stride_words] (bm_stride_words * 32 >= n),
 * removed int32 [n], ZERO on entry: removed[r] becomes the number of bits of row r that this call turned off.  Work items
 * are chunks of at most 256 elements of the enumerated (old) row, scheduled as in ocn_bitrows_insert: a hub row is spread
 * over many waves.  Every lane holds one candidate; only a bit that is set is decided: by its lane alone where the shorter
 * of the two lists has at most 32 columns (a guess, not measured), else by the whole wave striding the shorter list.  A bit
 * without a witness is cleared with 32-bit atomicAnd and counts exactly when the returned word still had it; the decision
 * reads A' only, which nothing writes, so bits and counts do not depend on scheduling.  Rows and columns outside [0, n) are
 * skipped.  workspace: ocn_bitrows_remove_workspace_bytes(nnzD) bytes, any content (16-byte aligned).
 * NULL pointers, n < 0, nnzD < 0 or >= 2^30, a stride too short: OCN_EINVAL before any HIP call.  n == 0 or nnzD == 0 returns 0. */
int64_t ocn_bitrows_remove_workspace_bytes(int64_t nnzD);
int ocn_bitrows_remove(const int64_t* rowptrA0, const int32_t* colA0, const int64_t* rowptrT0, const int32_t* colT0,
                       const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT, const int32_t* colT,
                       const int64_t* rowptrD, const int32_t* colD, int64_t n, int64_t nnzD, uint32_t* bits,
                       int64_t bm_stride_words, int32_t* removed, void* workspace, void* stream);

/* Which rows an edge update can reach (ocn_amd.update.EncoderState): the closed neighbourhood of a row list, as bits.
 *
 * ocn_rows_neighbourhood: (rowptrT, colT) = the n x n CSR whose row k lists the rows that READ column k — the transpose of the
 * adjacency, the adjacency itself where it is symmetric.  rows = int64 [n_list] (any order, duplicates allowed; an id outside
 * [0, n) is skipped).  bits = ONE bit row, uint32 [ceil(n / 32)], owned by the caller and OR-ed into, never cleared: on return
 * the bit of every listed row and of every column of those rows is set (32-bit atomicOr, as ocn_bitrows_insert sets its bits).
 * Work items are chunks of at most 256 row elements, scheduled by a scan of ceil(len / 256) as in ocn_bitrows_insert: a hub row
 * is spread over many waves.  workspace: ocn_rows_neighbourhood_workspace_bytes(n_list) bytes, any content (16-byte aligned).
 * NULL pointers, n < 0, n_list < 0 or >= 2^30: OCN_EINVAL before any HIP call.  n == 0 or n_list == 0 returns 0.
 *
 * ocn_bitlist_count / ocn_bitlist_fill: one bit row of n_bits bits as the ascending list of its set bits' ids, a thread per
 * word (ocn_bitrows_count / _fill walk a row on one wave: right for many rows, serial for one long one).  count (int32
 * [ceil(n_bits / 32)], the population of each word, bits at or past n_bits ignored) -> ocn_scan_i32 -> fill (out int64 [total],
 * word w's ids from out[off[w]] on; nothing is written at or past off[w + 1]).  NULL pointers or n_bits < 0: OCN_EINVAL before
 * any HIP call.  n_bits == 0 returns 0. */
int64_t ocn_rows_neighbourhood_workspace_bytes(int64_t n_list);
int ocn_rows_neighbourhood(const int64_t* rowptrT, const int32_t* colT, int64_t n, const int64_t* rows, int64_t n_list,
                           uint32_t* bits, void* workspace, void* stream);
int ocn_bitlist_count(const uint32_t* bits, int64_t n_bits, int32_t* count, void* stream);
int ocn_bitlist_fill(const uint32_t* bits, int64_t n_bits, const int64_t* off /* [words + 1], from ocn_scan_i32 */, int64_t* out,
                     void* stream);

/* Glue for head layouts the fused Linear kernel below does not cover (widths outside 32..256, training
 * mode; model.py:2203-2235, 2429-2437): y = LayerNorm(x) (eps, affine gamma/beta) followed by ReLU when `relu` != 0,
 * one pass over [rows][H] (replaces nn.LayerNorm + Dropout(eval) + nn.ReLU); and the branch mix
 * out = c[0]*x1 + c[1]*x2 + c[2]*x3 with the three coefficients read from device memory
 * (alpha.sigmoid().cumprod() and beta, model.py:2435-2436).  H in {16..512, power of two}. */
int ocn_rows_ln_relu(const float* x, const float* gamma, const float* beta, float eps, int32_t relu,
                     int64_t rows, int32_t H, float* y, void* stream);
int ocn_combine3(const float* coef, const float* x1, const float* x2, const float* x3, int64_t n,
                 float* out, void* stream);

/* The nn.Linear layers of the heads (model.py:2192-2235) on the matrix cores:
 *   Y[M][N] = epilogue(X[M][K] . W^T + bias),  X/W/Y fp32, W = nn.Linear.weight [N][K].
 * Each fp32 operand is split into three bf16 terms and the six leading cross products are
 * accumulated in fp32 on v_mfma_f32_32x32x16_bf16 (error below fp32's own rounding).
 * ocn_linear_split_weight writes the pre-split, fragment-ordered panel Wp
 * (ocn_linear_panel_bytes(N, K) bytes; redo it whenever W changes).  N in {32,64,128,256}, K % 16 == 0.
 * Epilogue, in this order: + bias (or NULL); LayerNorm over the N columns with gamma/beta/eps (or
 * both NULL); ReLU if relu != 0; then either store Y[M][N], or — when dotw != NULL — the trailing
 * Linear(N -> 1) of `lin`: Y[M] = <row, dotw> + dotb[0]. */
/* dst[row][0 .. n_cols) = vec[0 .. n_cols) for the rows of a device-side range (clamped to max_rows): the
 * constant activations of the candidates whose pooled input is all zero (ocn_class_order). */
int ocn_fill_rows(float* dst, int64_t ld, int32_t n_cols, const float* vec, const int64_t* row_range,
                  int64_t max_rows, void* stream);

/* Refused (-1), never dropped: `addend` together with `dotw` (the dot epilogue stores one float per row and adds
 * nothing), `y_row_map` without `dotw`, and an X, a stored Y (no `dotw`) or an addend that is not 16-byte aligned (rows
 * are read and written as float4; the row strides are multiples of 4 floats).  N is checked for a launch without rows too. */
typedef struct OcnLinearGroup {
  const float* X; int64_t ldX;       /* input [M][K], row stride in floats (0 = K) */
  int64_t M;
  const void* Wp;                    /* panel of this group's weight */
  const float* bias;                 /* or NULL */
  const float* gamma; const float* beta; float eps;   /* LayerNorm, or both NULL */
  int32_t relu;
  const float* scale;                /* device float[1] multiplied in after ReLU, or NULL */
  const float* addend; int64_t ldAdd;/* [M][N] added last (row stride, 0 = N), or NULL */
  const float* dotw; const float* dotb;   /* trailing Linear(N -> 1): Y is [M]; or NULL */
  float* Y; int64_t ldY;             /* output rows, row stride in floats (0 = N) */
  /* Rows [row_range[0], row_range[1]) of the M-row buffers only (device int64[2], clamped to [0, M]), or
   * NULL for all M rows: the bounds stay on the device, e.g. the class boundaries of a batch sorted by
   * "has common neighbours" (ocn_class_order) — no host sync to launch on a sub-range. */
  const int64_t* row_range;
  const int64_t* y_row_map;          /* dot epilogue only: Y[y_row_map[row]] instead of Y[row], or NULL */
  int32_t add_bcast;                 /* != 0: addend is ONE row [N] added to every row */
} OcnLinearGroup;

int64_t ocn_linear_panel_bytes(int32_t N, int32_t K);
int ocn_linear_split_weight(const float* W, int32_t N, int32_t K, void* Wp, void* stream);
int ocn_linear_bf16x6(const float* X, int64_t M, int32_t K, const void* Wp, int32_t N,
                      const float* bias, const float* gamma, const float* beta, float eps,
                      int32_t relu, const float* dotw, const float* dotb, float* Y, void* stream);
/* Up to 5 independent Linear layers of the same (K, N) in ONE launch (e.g. the first layers of
 * xcn1lin, xcn2lin and xijlin): more workgroups than CU slots, so one group's LayerNorm epilogue
 * overlaps another's MFMA loop, and strided outputs let two branches write the halves of a
 * [M][2N] buffer that a K = 2N Linear then consumes (the branch mix of model.py:2436 folded into
 * its weights).  `groups` is a HOST array. */
int ocn_linear_grouped(const OcnLinearGroup* groups, int32_t n_groups, int32_t K, int32_t N, void* stream);

/* The MLP heads of cn5 / cn7 (model.py:2203-2235, 2429-2437 == 3216-3223) as one launch per candidate batch:
 *   a = ReLU(LN(W3a ReLU(W0a xcn1 + b0a) + b3a)),  b likewise from xcn2,  c = ReLU(LN(W0x (x_i*x_j) + b0x)),
 *   y = Linear(H,1)(ReLU(LN(Ma a + Mb b + Mc c + bf)))
 * where the host has folded the reference's products without a non-linearity between them — the third layers
 * of xcn1lin / xcn2lin, the second layer of xijlin, the mix alpha0*xcn1 + alpha1*xcn2 + beta*xij (model.py:2436)
 * and lin[0] — into Ma, Mb, Mc, bf.  Every activation stays in registers; only x[3] is read and y written.
 * An f32 product is three f16 MFMAs on hi/lo splits of both operands (v_mfma_f32_32x32x16_f16, fp32 accumulate):
 * ocn_heads_split_weight writes the panel of scale * W (scale = a power of two that puts max |W| into
 * [2^13, 2^14); ocn_heads_panel_bytes(N, K) bytes) in the k order in which the previous layer's accumulator
 * registers arrive; activation rows are scaled per row inside the kernel.
 * p_first: panels of xcn1lin.0, xcn2lin.0, xijlin.0; p_mid: of xcn1lin.3, xcn2lin.3; p_out: of Ma, Mb, Mc.
 * vec: ocn_heads_nvec() vectors of H floats — b0a b3a g3a e3a  b0b b3b g3b e3b  b0x gx ex  bf gl el  dotw  constA constB
 * — followed by ocn_heads_nscal() scalars: the dot bias, then 1 / scale of the eight panels in the order
 * xcn1lin.0 xcn1lin.3 Ma xcn2lin.0 xcn2lin.3 Mb xijlin.0 Mc, then zeros (constA / constB are unused since ABI 6).
 * What a skipped branch contributes — Ma a, Mb b of an all-zero pooled row — comes from this entry in constants mode
 * (dump != NULL, B == 1, x = one zero row: fills ocn_heads_const_bytes(H) bytes, no score) and is handed back as
 * `cpark` in scoring mode.  ranges (or NULL) = ocn_class_order's table: the candidates then come class-major and a
 * workgroup without any cn1 (cn2) row adds the constant instead of running the branch; b_on_union: cn5 (xcn2 lives on
 * cn1 u cn2) vs cn7 (cn2 only).  H in {128, 256}; in_channels == H (narrower heads: ocn_linear_grouped). */
typedef struct OcnHeadsArgs {
  const float* x[3];
  int64_t ldx, B;
  int32_t H;
  const void* p_first[3];
  const void* p_mid[2];
  const void* p_out[3];
  const float* vec;
  const int64_t* ranges;
  const int64_t* y_row_map;
  float* y;
  float* dump;               /* constants mode: ocn_heads_const_bytes(H) bytes out, B == 1 */
  const float* cpark;        /* scoring mode: the buffer a constants-mode call filled */
  float* scratch;            /* ocn_heads_scratch_bytes(H) bytes: where a wave parks a finished branch's share of the output */
  float eps;
  int32_t ln, b_on_union;
} OcnHeadsArgs;
int32_t ocn_heads_nvec(void);
int32_t ocn_heads_nscal(void);
int64_t ocn_heads_scratch_bytes(int32_t H);
int64_t ocn_heads_const_bytes(int32_t H);
int64_t ocn_heads_panel_bytes(int32_t N, int32_t K);
int ocn_heads_split_weight(const float* W, int32_t N, int32_t K, float scale, void* Wp, void* stream);
int ocn_heads_fused(const OcnHeadsArgs* args, void* stream);
/* Batches of up to `max_rows` candidates are scored by the small-batch form of the same head — 32 candidates per workgroup,
 * the four waves splitting every layer's output features — which returns the same bits as the throughput form at a fifth of
 * its latency (Cora's 1 152-candidate batch: nine 128-row tiles = 70 us whatever the batch size).  Sets the bound (process-wide;
 * default 16384 = two rounds of workgroups on 256 CUs; quoted at H = 256 — at H = 128 twice as many rows take the small form) and
 * returns the previous one; a negative argument only queries. */
int64_t ocn_heads_small_batch(int64_t max_rows);

/* Training-side pieces (NeighborOverlap_large.py:56-63, 76-90).
 *
 * ocn_coo_to_csr: the per-batch masked adjacency — SparseTensor.from_edge_index(tei, sparse_sizes) (a sort by (row, col)
 * in torch_sparse; dedupe = 0: duplicates are kept, as there) and .to_symmetric() (symmetrize = 1, dedupe = 1: the
 * transposed entries join and the pattern is coalesced), pattern only.  Count -> scan -> fill -> per-row sort (wave rank
 * sort / workgroup bitonic network) -> unique count -> scan -> compact, all on `stream`.  rowptr [n_rows + 1]; col_out must
 * hold nnz * (symmetrize ? 2 : 1) entries (the upper bound); result[0] = entries written (= rowptr[n_rows]), result[1] = 1
 * if an index was out of range (such entries are dropped) — device memory, the caller reads it when it needs to. */
int64_t ocn_coo_to_csr_workspace_bytes(int64_t nnz, int64_t n_rows, int32_t symmetrize, int32_t dedupe);
int ocn_coo_to_csr(const int64_t* row, const int64_t* col, int64_t nnz, int64_t n_rows, int64_t n_cols,
                   int32_t symmetrize, int32_t dedupe, int64_t* rowptr, int32_t* col_out, void* workspace,
                   int64_t* result, void* stream);

/* ocn_wgrad: weight / bias gradient of a Linear layer, dW[N][K] = dY^T X, db[N] = column sums of dY (db may be NULL),
 * dY [B][N] row stride ldY, X [B][K] row stride ldX, fp32.  bf16x6 on the matrix cores, split over the batch; the
 * slices' partial results are added in slice order (no float atomics: the same bits on every run).  Any N, K >= 1. */
int64_t ocn_wgrad_workspace_bytes(int64_t B, int32_t N, int32_t K);
int ocn_wgrad(const float* dY, int64_t ldY, const float* X, int64_t ldX, int64_t B, int32_t N, int32_t K,
              float* dW, float* db, void* workspace, void* stream);

/* The heads' LayerNorm -> Dropout -> ReLU tails under autograd (the nn.Sequential layouts of model.py:2203-2235 in train(),
 * NeighborOverlap_large.py:76-90), one forward and two backward launches:
 *   y = relu?( dropout_p( gamma == NULL ? x : LN(x; gamma, beta, eps) ) ),   x, y [rows][H] fp32, H in {16 .. 512}
 * stats (with gamma): float[rows][2] = {mean, 1 / sqrt(var + eps)} for the backward.  Dropout keeps an element iff a
 * counter-based hash of (seed, element index) passes p — no mask is stored; the backward recomputes it from the same seed
 * (ocn_dropout_keep_mask exposes the decisions for tests).  This is the library's random stream, not torch's.
 * backward: dx; with gamma also dgamma / dbeta — every one of a FIXED number of lane groups walks a contiguous block of rows
 * and keeps its own partial sums, a second launch adds them in block order: the same bits on every run.
 * workspace: ocn_ln_drop_relu_workspace_bytes(H) (with gamma). */
int64_t ocn_ln_drop_relu_workspace_bytes(int32_t H);
int ocn_ln_drop_relu_forward(const float* x, const float* gamma /* or NULL */, const float* beta /* or NULL */, float eps, float p,
                             uint64_t seed, int32_t relu, int64_t rows, int32_t H, float* y, float* stats /* [rows][2], with gamma */,
                             void* stream);
int ocn_ln_drop_relu_backward(const float* g, const float* x, const float* y, const float* stats, const float* gamma /* or NULL */,
                              float p, uint64_t seed, int32_t relu, int64_t rows, int32_t H, float* dx,
                              float* dgamma, float* dbeta, void* workspace, void* stream);
int ocn_dropout_keep_mask(uint64_t seed, float p, int64_t n, uint8_t* out, void* stream);

/* Backward of the branch mix z = coef[0] x1 + coef[1] x2 + coef[2] x3 (ocn_combine3; model.py:2436, 3222): d_k = coef[k] g and
 * dcoef[k] = <g, x_k> — per-workgroup partial sums over contiguous chunks, added in workgroup order (deterministic).  n a
 * multiple of 4; workspace: ocn_mix3_workspace_bytes(). */
int64_t ocn_mix3_workspace_bytes(void);
int ocn_mix3_backward(const float* coef, const float* g, const float* x1, const float* x2, const float* x3, int64_t n,
                      float* d1, float* d2, float* d3, float* dcoef, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCN_HIP_H */
