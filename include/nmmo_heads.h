/*
 * nmmo_heads.h — C-ABI of the fused masked action heads (libnmmo_heads.so).
 *
 * Every policy of the reference ends in the same step (baseline_policy.py:245-262): per action
 * head, masked_fill(mask == 0, -1e9) on the head's logits, a Categorical, then sample / log_prob
 * / entropy. nmh_forward does that for all heads of a row in one gfx950 kernel, reading the mask
 * in place from the obs row; nmh_backward is its gradient with respect to the logits. The
 * semantics are frozen in SPEC.md §15. nmh_pointer_forward / nmh_pointer_backward do the same for
 * heads whose logits are dot products of a query with candidate keys (SPEC.md §18).
 *
 * Conventions (those of nmmo_hip.h): every call returns 0 or a negative NMH_E_* code and never
 * aborts; nmh_last_error() returns a thread-local message. Argument errors are reported without
 * touching a GPU. Every buffer is a caller-owned DEVICE pointer; work is enqueued on `stream`
 * (a hipStream_t, NULL = default stream) with no synchronisation and no allocation inside.
 */
#ifndef NMMO_HEADS_H
#define NMMO_HEADS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMH_API __attribute__((visibility("default")))

#define NMH_OK 0
#define NMH_E_INVALID (-1) /* bad argument */
#define NMH_E_HIP (-2)     /* HIP runtime error */

#define NMH_MAX_HEADS 16
#define NMH_MAX_DIM 2048

/* The heads of one row, concatenated: head k is dims[k] consecutive entries of a logits row and
 * of a mask row. 1 <= n_heads <= NMH_MAX_HEADS, 1 <= dims[k] <= NMH_MAX_DIM. */
typedef struct NmhHeads {
  int32_t n_heads;
  int32_t dims[NMH_MAX_HEADS];
} NmhHeads;

#define NMH_MASK_F32 0 /* float32 mask, legal iff value > 0 (the flat obs row's prefix) */
#define NMH_MASK_U8 1  /* byte mask, legal iff byte != 0 (native obs row, bool tensors) */

/* Strides are in elements of the row's type and must be >= sum(dims). Rows need no alignment.
 *
 * actions_in NULL: sample (seed, offset, row_base select the draws: row r, head k uses the
 * philox counter (row_base + r, k, offset)); else evaluate the given [n_rows, n_heads] actions.
 * actions_out [n_rows, n_heads] gets the sampled actions, or a copy of actions_in.
 * logprob / entropy [n_rows]: sums over heads. lse / head_entropy [n_rows, n_heads]: per head,
 * what nmh_backward needs. n_rows == 0 is a no-op. */
NMH_API int nmh_forward(const NmhHeads* hd, int32_t n_rows, const float* logits, int64_t logits_stride,
                        const void* mask, int64_t mask_stride, int32_t mask_kind, const int32_t* actions_in,
                        uint64_t seed, uint64_t offset, uint32_t row_base, int32_t* actions_out,
                        float* logprob, float* entropy, float* lse, float* head_entropy, void* stream);

/* d(sum_r g_logprob[r] logprob[r] + g_entropy[r] entropy[r]) / d logits into g_logits (row stride
 * g_stride >= sum(dims)); every entry of the sum(dims) prefix of every row is written, zeros
 * included. g_logprob / g_entropy [n_rows]; either may be NULL (= zeros). */
NMH_API int nmh_backward(const NmhHeads* hd, int32_t n_rows, const float* logits, int64_t logits_stride,
                         const void* mask, int64_t mask_stride, int32_t mask_kind, const int32_t* actions,
                         const float* lse, const float* head_entropy, const float* g_logprob,
                         const float* g_entropy, float* g_logits, int64_t g_stride, void* stream);

/* ---- Pointer heads (SPEC.md §18): a head whose logits are dot products of a per-row query with
 * per-row candidate keys, as the reference's decoders compute them (baseline_policy.py:222-230),
 * fused with the masked categorical above. The logits are never materialised, and the key rows of
 * illegal candidates are never read. */
#define NMH_MAX_SETS 4
#define NMH_MAX_KEY_DIM 256

/* head_set[k] = -1: head k is dense, its dims[k] logits are given. head_set[k] = s in
 * [0, n_sets): head k points into key set s, which has set_rows[s] >= 1 candidates per row, and
 * dims[k] == set_rows[s] + 1: the last entry is the no-op, whose logit is exactly 0 (the
 * reference's zero padding row). 0 <= n_sets <= NMH_MAX_SETS and every set is used by a head.
 * key_dim (D) is a multiple of 4 in 4..NMH_MAX_KEY_DIM; it is not looked at when n_sets == 0.
 * sum(dims) <= NMH_MAX_DIM. */
typedef struct NmhPointer {
  int32_t n_sets;
  int32_t key_dim;
  int32_t set_rows[NMH_MAX_SETS];
  int32_t head_set[NMH_MAX_HEADS];
} NmhPointer;

/* queries [n_rows, P, D]: one query per pointer head, P = the number of pointer heads, in head
 * order (NULL iff P == 0). keys: a HOST array of n_sets device pointers, keys[s] [n_rows,
 * set_rows[s], D] (NULL iff n_sets == 0). Queries and keys are contiguous and 16-byte aligned.
 * dense [n_rows, dense_stride]: the dense heads' logits concatenated in head order, dense_stride
 * >= their total (NULL iff no head is dense). mask rows cover all heads as in nmh_forward.
 * The remaining arguments and every output are those of nmh_forward. */
NMH_API int nmh_pointer_forward(const NmhHeads* hd, const NmhPointer* pt, int32_t n_rows, const float* queries,
                                const float* const* keys, const float* dense, int64_t dense_stride,
                                const void* mask, int64_t mask_stride, int32_t mask_kind,
                                const int32_t* actions_in, uint64_t seed, uint64_t offset, uint32_t row_base,
                                int32_t* actions_out, float* logprob, float* entropy, float* lse,
                                float* head_entropy, void* stream);

/* The gradient of sum_r g_logprob[r] logprob[r] + g_entropy[r] entropy[r]: g_dense [n_rows,
 * g_dense_stride] like nmh_backward's g_logits over the dense heads, g_queries like queries,
 * g_keys a HOST array of n_sets device pointers, g_keys[s] like keys[s] (16-byte aligned). Any of
 * g_dense, g_queries, g_keys and each g_keys[s] may be NULL: that gradient is not computed. Every
 * entry of every other one is written, zeros included; no atomics, the same bits on every run. */
NMH_API int nmh_pointer_backward(const NmhHeads* hd, const NmhPointer* pt, int32_t n_rows, const float* queries,
                                 const float* const* keys, const float* dense, int64_t dense_stride,
                                 const void* mask, int64_t mask_stride, int32_t mask_kind,
                                 const int32_t* actions, const float* lse, const float* head_entropy,
                                 const float* g_logprob, const float* g_entropy, float* g_dense,
                                 int64_t g_dense_stride, float* g_queries, float* const* g_keys, void* stream);

/* ---- Tile encoder (SPEC.md §19): the embedding, the first 3x3 convolution and the ReLU of the
 * reference's TileEncoder (baseline_policy.py:95-107) as one lookup into a table folded from the
 * two layers' weights, table[f][v][k][o] = sum_e W1[o][f*32 + e][ky][kx] E[f*256 + v][e], k = ky*3 + kx.
 * The shape is the start-kit policy's. */
#define NMH_TILE_TILES 225    /* 15 x 15 tiles per row, in order t = y*15 + x */
#define NMH_TILE_FEATURES 3   /* (row, col, material) per tile */
#define NMH_TILE_VALUES 256   /* embedding rows per feature */
#define NMH_TILE_TAPS 9       /* 3 x 3 */
#define NMH_TILE_CHANNELS 32  /* output channels */
#define NMH_TILE_OUT 169      /* 13 x 13 output positions per channel */
#define NMH_TILE_FWD_ROWS 4   /* rows per workgroup of the forward kernel */
#define NMH_TILE_MAX_CHUNKS 64

#define NMH_TILE_F32 0 /* float32 Tile section (the flat obs row) */
#define NMH_TILE_I16 1 /* int16 Tile section (the native obs row) */

/* tile: row r's Tile section, 675 entries (row, col, material) x 225 read in place at
 * tile + r * tile_stride elements of the kind's type; tile_stride >= 675, rows need no alignment
 * beyond their element's, and the input is never written. idx[t][f] = clamp(trunc(v), 0, 255) with
 * v = (tile[t][f] - tile[112][f]) + 7 for f < 2 (float32: two roundings; NaN gives 0) and
 * v = tile[t][2] for the material.
 * out [n_rows, 32, 13, 13] = max(0, bias[o] + sum over ky, kx, f in that order of
 * table[f][idx[(y+ky)*15 + x+kx][f]][ky*3+kx][o]), float32 without contraction.
 * table [3, 256, 9, 32] and bias [32] are 16-byte aligned. idx_out: NULL, or uint8 [n_rows, 225, 3]
 * that receives idx (what nmh_tile_backward reads). */
NMH_API int nmh_tile_forward(int32_t n_rows, const void* tile, int64_t tile_stride, int32_t tile_kind,
                             const float* table, const float* bias, float* out, uint8_t* idx_out, void* stream);

/* The gradient with respect to table and bias, given idx and out as nmh_tile_forward stored them
 * and g_out like out (out and g_out contiguous and 16-byte aligned). Chunk c of n_chunks
 * (1..NMH_TILE_MAX_CHUNKS) covers rows [c R, min(n_rows, (c+1) R)), R = ceil(n_rows / n_chunks);
 * g_table_parts [n_chunks, 3, 256, 9, 32] and g_bias_parts [n_chunks, 32] receive each chunk's
 * sums, every entry written (an empty chunk's are zeros), and the caller adds the chunks. No
 * atomics: the same bits on every run for a given (n_rows, n_chunks). */
NMH_API int nmh_tile_backward(int32_t n_rows, const uint8_t* idx, const float* out, const float* g_out,
                              int32_t n_chunks, float* g_table_parts, float* g_bias_parts, void* stream);

/* ---- Tile encoder with the second convolution (SPEC.md §22): a1 = relu(conv1(embed(tile))) as
 * above, kept on chip, then the reference's tile_conv_2 (32 -> 8 channels, 3 x 3) and its ReLU
 * (baseline_policy.py:108). Only out2 [n_rows, 8, 11, 11], what tile_fc consumes, is written. */
#define NMH_TILE2_CHANNELS 8     /* output channels of tile_conv_2 */
#define NMH_TILE2_OUT 121        /* 11 x 11 output positions per channel */
#define NMH_TILE2_FWD_ROWS 4     /* rows per workgroup of the forward kernel */
#define NMH_TILE2_MAX_PARTS 1024 /* parts of rows whose g_w2 and g_bias2 are summed separately */

/* tile, tile_stride, tile_kind, table, bias1 and idx_out as for nmh_tile_forward; a1 is its `out`,
 * bit for bit, and is never stored. w2 [8, 32, 3, 3] and bias2 [8] are tile_conv_2's weight and bias,
 * 16-byte aligned like table and bias1.
 * out2[n][o2][y][x] = max(0, z), z = bias2[o2], then for c in 0..31, ky in 0..2, kx in 0..2 in that
 * order z += w2[o2][c][ky][kx] * a1[n][c][y+ky][x+kx]: one float32 multiply and one float32 add per
 * term, no contraction. out2 is contiguous and needs no alignment beyond a float's. */
NMH_API int nmh_tile2_forward(int32_t n_rows, const void* tile, int64_t tile_stride, int32_t tile_kind,
                              const float* table, const float* bias1, const float* w2, const float* bias2,
                              float* out2, uint8_t* idx_out, void* stream);

/* The gradients with respect to table, bias1, w2 and bias2, given idx and out2 as nmh_tile2_forward
 * stored them, g_out2 like out2, and the forward's table, bias1 and w2 (16-byte aligned): a1 is
 * recomputed from them. Two launches. The first takes part g of n_w2_parts (1..NMH_TILE2_MAX_PARTS),
 * rows [g R, min(n_rows, (g+1) R)), R = ceil(n_rows / n_w2_parts), per workgroup: with
 * dz2 = g_out2 where out2 > 0 and 0 elsewhere it writes
 * dz1[n][c][y][x] = (a1 > 0) * sum over o2, ky, kx of w2[o2][c][ky][kx] * dz2[n][o2][y-ky][x-kx]
 * to dz1_scratch [n_rows, 32, 13, 13] (16-byte aligned; transient, the caller neither fills nor
 * reads it) and the part's sums to g_w2_parts [n_w2_parts, 8, 32, 3, 3] and g_bias2_parts
 * [n_w2_parts, 8]. The second is nmh_tile_backward's kernel over dz1: n_table_chunks,
 * g_table_parts [n_table_chunks, 3, 256, 9, 32] and g_bias1_parts [n_table_chunks, 32] as there.
 * Every entry of every part is written (an empty part's are zeros) and the caller adds the parts.
 * No atomics: the same bits on every run for a given (n_rows, n_table_chunks, n_w2_parts). */
NMH_API int nmh_tile2_backward(int32_t n_rows, const uint8_t* idx, const float* out2, const float* g_out2,
                               const float* table, const float* bias1, const float* w2, int32_t n_table_chunks,
                               int32_t n_w2_parts, float* dz1_scratch, float* g_table_parts, float* g_bias1_parts,
                               float* g_w2_parts, float* g_bias2_parts, void* stream);

/* ---- Item encoder (SPEC.md §20): the reference's ItemEncoder (baseline_policy.py:148-170) is a
 * linear layer over a fixed 32-feature function x of an item's 16 columns, so its mean pool needs
 * only the sum of x over a set, and a pointer logit q . fc(x_j) = (W^T q) . x_j + q . b needs only
 * candidate j's own columns. No embedding tensor is made.
 * x[i] = (i == t), i < 18, t = clamp(trunc(col 1), 0, 17); x[18 + i] = (i == e), i < 2,
 * e = clamp(trunc(col 14), 0, 1); NaN gives class 0; x[20 + k] = col cont[k] * 0.01f, one float32
 * product, cont = 3, 4, ..., 13, 15. */
#define NMH_ITEM_COLS 16
#define NMH_ITEM_FEATURES 32
#define NMH_ITEM_TYPES 18
#define NMH_ITEM_QUERY 36      /* floats per projected query: 32 weights, the constant, 3 pads */
#define NMH_ITEM_MAX_ROWS 1024 /* items per set */
#define NMH_ITEM_MAX_HEADS 4   /* heads over one set per call */

#define NMH_ITEM_F32 0 /* float32 item columns (the flat obs row) */
#define NMH_ITEM_I16 1 /* int16 item columns (the native obs), converted exactly */

/* items: set m's R x 16 item columns read in place at items + m * item_stride elements of the kind's
 * type (item_stride >= 16 R; rows need no alignment beyond their element's; never written).
 * features [n_sets, R, 32] and sums [n_sets, 32]: either may be NULL, not both.
 * sums[f] = the number of items of the class, f < 20 (exact); sums[20 + k] = (sum over the set's items of
 * col cont[k], in one fixed order) * 0.01f. 1 <= R = set_rows <= NMH_ITEM_MAX_ROWS; n_sets == 0 is a no-op. */
NMH_API int nmh_item_features(int32_t n_sets, const void* items, int64_t item_stride, int32_t item_kind,
                              int32_t set_rows, float* features, float* sums, void* stream);

typedef struct NmhSetHeads { /* 1..NMH_ITEM_MAX_HEADS heads over one candidate set, items or entities */
  int32_t n_heads;
  int32_t mask_off[NMH_ITEM_MAX_HEADS]; /* head h's first of set_rows + 1 entries in a mask row */
  int32_t out_off[NMH_ITEM_MAX_HEADS];  /* ... and in an out / g_out row */
} NmhSetHeads;
typedef NmhSetHeads NmhItemHeads; /* 1..NMH_ITEM_MAX_HEADS heads over one item set */

/* Obs row r reads item set r / share (share >= 1: 1 for flat rows, P for the native per-env Market).
 * pq [n_rows, n_heads, 36], 16-byte aligned. out [n_rows, out_stride]. Mask as in nmh_forward; both
 * strides cover the furthest head's set_rows + 1 entries.
 * out[r][out_off[h] + j], j < R legal: v = pq[32] + pq[t]; v += pq[18 + e]; v = fmaf(pq[20 + k], x[20 + k], v),
 * k = 0..11. Illegal j and the no-op j = R: 0.0f. All R + 1 entries are written, nothing else is, and
 * the items of illegal candidates are never read. n_rows == 0 is a no-op. */
NMH_API int nmh_item_logits(const NmhItemHeads* ih, int32_t n_rows, const void* items, int64_t item_stride,
                            int32_t item_kind, int32_t set_rows, int32_t share, const void* mask,
                            int64_t mask_stride, int32_t mask_kind, const float* pq, float* out,
                            int64_t out_stride, void* stream);

/* g_pq [n_rows, n_heads, 36]: g_pq[f] = fmaf(g_out[j], (x_j, 1)[f], .) over the legal j < R in
 * ascending order, f < 33; the three pads are written as 0. g_out [n_rows, g_stride] like out; its
 * entries of illegal candidates and of the no-op are not read. No atomics: the same bits on every run. */
NMH_API int nmh_item_logits_backward(const NmhItemHeads* ih, int32_t n_rows, const void* items, int64_t item_stride,
                                     int32_t item_kind, int32_t set_rows, int32_t share, const void* mask,
                                     int64_t mask_stride, int32_t mask_kind, const float* g_out, int64_t g_stride,
                                     float* g_pq, void* stream);

/* ---- Player encoder (SPEC.md §21): the reference's PlayerEncoder (baseline_policy.py:115-145) is
 * two linear layers over a fixed 35-feature function x of an entity's 31 columns, so the mean pool
 * of agent_fc needs only the sum of x over a row's entities, a pointer logit q . agent_fc(x_j) =
 * (W^T q) . x_j + q . b needs only candidate j's own columns, and my_agent_fc needs x of one entity.
 * No embedding tensor is made.
 * x[0] = col 0; x[1 + i] = (i == t), i < 5, t = clamp(trunc(col 1), 0, 4), NaN gives 0;
 * x[6 + k] = col (2 + k), k < 29. No column is scaled. */
#define NMH_PLAYER_COLS 31
#define NMH_PLAYER_FEATURES 35
#define NMH_PLAYER_TYPES 5
#define NMH_PLAYER_QUERY 40     /* floats per projected query: 35 weights, the constant, 4 pads */
#define NMH_PLAYER_MAX_ROWS 256 /* entities per set */
#define NMH_PLAYER_MAX_HEADS 4  /* heads over one set per call */

#define NMH_PLAYER_F32 0 /* float32 elements (the flat obs row) */
#define NMH_PLAYER_I16 1 /* int16 elements (the native obs), converted exactly */

/* ents: set m's R x 31 entity columns read in place at ents + m * ent_stride elements of ent_kind's
 * type (ent_stride >= 31 R; rows need no alignment beyond their element's; never written).
 * ids: set m's AgentId read in place at ids + m * id_stride elements of id_kind's type (id_stride >= 1).
 * features [n_sets, R, 35], sums [n_sets, 35], mine [n_sets, 35], mine_idx int32 [n_sets]: any may be
 * NULL, not all four; ids may be NULL only if mine and mine_idx both are.
 * sums[0], sums[6 + k] = the float32 sum of the raw column in one fixed order; sums[1 + i] = the number
 * of entities of class i (exact). mine_idx[m] = the smallest j < R with col 0 == id and col 0 != 0,
 * else 0 (a NaN id matches nothing); mine[m] = x of that entity.
 * 1 <= R = set_rows <= NMH_PLAYER_MAX_ROWS; n_sets == 0 is a no-op. */
NMH_API int nmh_player_features(int32_t n_sets, const void* ents, int64_t ent_stride, int32_t ent_kind,
                                int32_t set_rows, const void* ids, int64_t id_stride, int32_t id_kind,
                                float* features, float* sums, float* mine, int32_t* mine_idx, void* stream);

#if NMH_ITEM_MAX_HEADS != NMH_PLAYER_MAX_HEADS
#error "NmhSetHeads serves item and entity sets: NMH_ITEM_MAX_HEADS must equal NMH_PLAYER_MAX_HEADS"
#endif
typedef NmhSetHeads NmhPlayerHeads; /* 1..NMH_PLAYER_MAX_HEADS heads over one entity set */

/* Obs row r reads entity set r. pq [n_rows, n_heads, 40], 16-byte aligned. out [n_rows, out_stride].
 * Mask as in nmh_forward; both strides cover the furthest head's set_rows + 1 entries.
 * out[r][out_off[h] + j], j < R legal: v = pq[35] + pq[1 + t]; v = fmaf(pq[0], col 0, v);
 * v = fmaf(pq[6 + k], col (2 + k), v), k = 0..28. Illegal j and the no-op j = R: 0.0f. All R + 1
 * entries are written, nothing else is, and an entity that no head of the call allows is never
 * read. n_rows == 0 is a no-op. */
NMH_API int nmh_player_logits(const NmhPlayerHeads* ph, int32_t n_rows, const void* ents, int64_t ent_stride,
                              int32_t ent_kind, int32_t set_rows, const void* mask, int64_t mask_stride,
                              int32_t mask_kind, const float* pq, float* out, int64_t out_stride, void* stream);

/* g_pq [n_rows, n_heads, 40]: g_pq[f] = fmaf(g_out[j], (x_j, 1)[f], .) over the legal j < R in
 * ascending order, f < 36; the four pads are written as 0. g_out [n_rows, g_stride] like out; its
 * entries of illegal candidates and of the no-op are not read. No atomics: the same bits on every run. */
NMH_API int nmh_player_logits_backward(const NmhPlayerHeads* ph, int32_t n_rows, const void* ents,
                                       int64_t ent_stride, int32_t ent_kind, int32_t set_rows, const void* mask,
                                       int64_t mask_stride, int32_t mask_kind, const float* g_out,
                                       int64_t g_stride, float* g_pq, void* stream);

/* ---- Embedded sets (SPEC.md §25): the takeru policy's ReducedPlayerEncoder and ReducedItemEncoder
 * are a linear layer over cat(E[idx_0], .., E[idx_{D-1}], x_0 / s_0, .., x_{C-1} / s_{C-1}) of a
 * candidate's columns: D discrete columns, idx_d = clip(trunc(x + off_d), 0, 255) with NaN giving 0,
 * and C continuous columns, x / s being one IEEE float32 division. The calls hold no parameters: the
 * caller folds a head's query into a score table pq (below) and reads back the table's gradient.
 *   NMH_EMBED_ENTITY: 31 columns. Discrete: columns 0, 1, 8, 10 with off 0, 256, 512, 768 (so the last
 *     three read bin 255 for every value >= -1, -257, -513). Continuous: columns 2..7, 9, 11..30 with
 *     s = 256, 256, 100, 1024, 3, 50, 1024, 100, 100, 100, 100, then (10, 100) seven times, then 100, 10.
 *   NMH_EMBED_ITEM: 16 columns. Discrete: columns 1, 14 with off 2, 0. Continuous: columns 3..13, 15
 *     with s = 10, 10, 10, 100, 100, 100, 40, 40, 40, 100, 100, 100.
 * Element kinds are NMH_ELEM_F32 / NMH_ELEM_I16; an int16 element is converted exactly first. */
#define NMH_EMBED_ENTITY 0
#define NMH_EMBED_ITEM 1
#define NMH_EMBED_BINS 256           /* table rows an index can reach */
#define NMH_EMBED_ENTITY_QUERY 1052  /* floats per score table: 4 x 256 bins, 27 weights, the bias */
#define NMH_EMBED_ITEM_QUERY 528     /* 2 x 256 bins, 12 weights, the bias, 3 pads */

/* set: set m's R x cols columns read in place at set + m * set_stride elements (set_stride >= cols R;
 * no alignment beyond the element's; never written). 1 <= R = set_rows <= NMH_PLAYER_MAX_ROWS (entity)
 * or NMH_ITEM_MAX_ROWS (item). Outputs, any of which may be NULL, not all:
 *   idx uint8 [n_sets, R, D] and cont float32 [n_sets, R, C]: every candidate's indices and x / s;
 *   counts float32 [n_sets, D, 256]: the number of the set's candidates with idx_d == i (exact);
 *   sums float32 [n_sets, C]: the float32 sum of the raw column, not divided, in one fixed order;
 *   mine_idx int32 [n_sets], mine_i uint8 [n_sets, D], mine_c float32 [n_sets, C] (entity kind only):
 *     the smallest j < R with col 0 == id and col 0 != 0, else 0, and that candidate's idx and cont;
 *     ids, id_stride, id_kind as in nmh_player_features, and ids may be NULL only if all three are.
 * n_sets == 0 is a no-op. */
NMH_API int nmh_embed_features(int32_t kind, int32_t n_sets, const void* set, int64_t set_stride, int32_t elem_kind,
                               int32_t set_rows, const void* ids, int64_t id_stride, int32_t id_kind, uint8_t* idx,
                               float* cont, float* counts, float* sums, int32_t* mine_idx, uint8_t* mine_i,
                               float* mine_c, void* stream);

/* Obs row r reads set r / share (share >= 1). pq [n_rows, n_heads, Q], 16-byte aligned, Q the kind's
 * *_QUERY: pq[256 d + i] scores index i of discrete column d, pq[256 D + c] weighs continuous column
 * c, pq[256 D + C] is the bias, the rest pads. out [n_rows, out_stride]; mask as in nmh_forward; both
 * strides cover the furthest head's set_rows + 1 entries.
 * out[r][out_off[h] + j], j < R legal: v = pq[256 D + C]; v += pq[256 d + idx_d], d ascending;
 * v = fmaf(x_c / s_c, pq[256 D + c], v), c ascending. Illegal j and the no-op j = R: 0.0f. All R + 1
 * entries are written, nothing else is, and a candidate that no head of the call allows is never
 * read. n_rows == 0 is a no-op. */
NMH_API int nmh_embed_logits(int32_t kind, const NmhSetHeads* sh, int32_t n_rows, const void* set,
                             int64_t set_stride, int32_t elem_kind, int32_t set_rows, int32_t share,
                             const void* mask, int64_t mask_stride, int32_t mask_kind, const float* pq, float* out,
                             int64_t out_stride, void* stream);

/* g_pq [n_rows, n_heads, Q]: over the head's legal j < R in ascending order, g_pq[256 d + i] = the
 * sum of g_out[j] where idx_d(j) == i, g_pq[256 D + c] = fmaf(g_out[j], x_c / s_c, .), g_pq[256 D + C]
 * = the sum of g_out[j]; the pads are written as 0. g_out [n_rows, g_stride] like out; its entries of
 * illegal candidates and of the no-op are not read. No atomics: the same bits on every run. */
NMH_API int nmh_embed_logits_backward(int32_t kind, const NmhSetHeads* sh, int32_t n_rows, const void* set,
                                      int64_t set_stride, int32_t elem_kind, int32_t set_rows, int32_t share,
                                      const void* mask, int64_t mask_stride, int32_t mask_kind, const float* g_out,
                                      int64_t g_stride, float* g_pq, void* stream);

/* ---- Decoder (SPEC.md §23): every action head of a row from the obs row itself, in one launch.
 * A head is dense (its logits are given) or a pointer head into one of up to NMH_MAX_SETS candidate
 * sets that are read in place; a pointer head's logits are §20's (item sets) or §21's (entity sets)
 * and go straight into the masked categorical of §15. The call equals, bit for bit,
 * nmh_forward / nmh_backward on the logits row that nmh_item_logits / nmh_player_logits and the dense
 * logits would make, with the *_logits_backward calls behind it; that row is never made. */
#define NMH_SET_ENTITY 0 /* SPEC §21: 31 columns, 35 features, 1..NMH_PLAYER_MAX_ROWS candidates */
#define NMH_SET_ITEM 1   /* SPEC §20: 16 columns, 32 features, 1..NMH_ITEM_MAX_ROWS candidates */
#define NMH_ELEM_F32 0   /* float32 candidate columns (the flat obs row) */
#define NMH_ELEM_I16 1   /* int16 candidate columns (the native obs), converted exactly */
#define NMH_DECODER_QUERY 40 /* floats per pointer head in pq and g_pq */

/* Set s has set_rows[s] = R candidates of rule[s]'s columns, read in place for obs row r at
 * base[s] + (r / share[s]) * stride[s] elements of elem_kind's type: stride[s] >= columns * R,
 * share[s] >= 1 (1 for flat rows, the players per env for the native per-env Market). One elem_kind
 * holds for all sets of a call; rows need no alignment beyond their element's and are never written.
 * head_set[k] = -1: head k is dense; else head k points into set head_set[k] and dims[k] == R + 1,
 * the last entry being the no-op whose logit is exactly 0.0f. 0 <= n_sets <= NMH_MAX_SETS, every
 * set is used by a head, and sum(dims) <= NMH_MAX_DIM. base holds DEVICE pointers. */
typedef struct NmhDecoderSets {
  int32_t n_sets;
  int32_t elem_kind;
  int32_t rule[NMH_MAX_SETS];
  int32_t set_rows[NMH_MAX_SETS];
  int32_t share[NMH_MAX_SETS];
  int32_t head_set[NMH_MAX_HEADS];
  int64_t stride[NMH_MAX_SETS];
  const void* base[NMH_MAX_SETS];
} NmhDecoderSets;

/* pq [n_rows, P, 40], 16-byte aligned: one slot per pointer head in head order (NULL iff P == 0). An
 * item head reads floats 0..32 of its slot as nmh_item_logits reads a projected query, an entity
 * head 0..35 as nmh_player_logits does; the rest of a slot is ignored. dense [n_rows, dense_stride]:
 * the dense heads' logits in head order (NULL iff no head is dense). mask, mask_stride, mask_kind,
 * actions_in, seed, offset, row_base and the five outputs are nmh_forward's. A candidate that its
 * head's mask forbids is never addressed. Dynamic LDS stays below 64 KiB: four rows per workgroup
 * where four waves fit (the nmmo heads: 63,040 bytes), else two. n_rows == 0 is a no-op. */
NMH_API int nmh_decoder_forward(const NmhHeads* hd, const NmhDecoderSets* sets, int32_t n_rows, const float* pq,
                                const float* dense, int64_t dense_stride, const void* mask, int64_t mask_stride,
                                int32_t mask_kind, const int32_t* actions_in, uint64_t seed, uint64_t offset,
                                uint32_t row_base, int32_t* actions_out, float* logprob, float* entropy,
                                float* lse, float* head_entropy, void* stream);

/* The gradient of sum_r g_logprob[r] logprob[r] + g_entropy[r] entropy[r] (either may be NULL = zeros):
 * g_dense [n_rows, g_dense_stride] like nmh_backward's g_logits over the dense heads, every entry
 * written, zeros included; g_pq like pq (16-byte aligned): g_pq[f] = fmaf(g_j, (x_j, 1)[f], .) over the
 * head's legal j < R in ascending order, g_j being nmh_backward's expression on the recomputed logit,
 * and the floats of a slot that forward ignores written as 0. g_dense or g_pq may be NULL: it is not
 * computed, and a head none of whose gradients is wanted is skipped. No atomics: the same bits on
 * every run. */
NMH_API int nmh_decoder_backward(const NmhHeads* hd, const NmhDecoderSets* sets, int32_t n_rows, const float* pq,
                                 const float* dense, int64_t dense_stride, const void* mask, int64_t mask_stride,
                                 int32_t mask_kind, const int32_t* actions, const float* lse,
                                 const float* head_entropy, const float* g_logprob, const float* g_entropy,
                                 float* g_dense, int64_t g_dense_stride, float* g_pq, void* stream);

/* ---- Greedy selection (SPEC.md §24): the three forward calls above with the draw replaced by the
 * argmax, for scoring a policy deterministically. Per head the action is the smallest index among
 * the legal entries whose logit equals the head's maximum; a head with no legal entry gives action 0
 * and contributes 0, as above. logprob, entropy, lse and head_entropy are, bit for bit, what the base
 * call returns for actions_in = the actions_out of this one, and the matching *_backward takes them.
 * Every other argument, check and limit is the base call's; there is no actions_in and no philox
 * counter. The selection is a compile-time parameter of the kernels: the base calls run the code
 * they ran before. n_rows == 0 is a no-op. */
NMH_API int nmh_forward_argmax(const NmhHeads* hd, int32_t n_rows, const float* logits, int64_t logits_stride,
                               const void* mask, int64_t mask_stride, int32_t mask_kind, int32_t* actions_out,
                               float* logprob, float* entropy, float* lse, float* head_entropy, void* stream);

NMH_API int nmh_pointer_forward_argmax(const NmhHeads* hd, const NmhPointer* pt, int32_t n_rows,
                                       const float* queries, const float* const* keys, const float* dense,
                                       int64_t dense_stride, const void* mask, int64_t mask_stride,
                                       int32_t mask_kind, int32_t* actions_out, float* logprob, float* entropy,
                                       float* lse, float* head_entropy, void* stream);

NMH_API int nmh_decoder_forward_argmax(const NmhHeads* hd, const NmhDecoderSets* sets, int32_t n_rows,
                                       const float* pq, const float* dense, int64_t dense_stride, const void* mask,
                                       int64_t mask_stride, int32_t mask_kind, int32_t* actions_out, float* logprob,
                                       float* entropy, float* lse, float* head_entropy, void* stream);

NMH_API const char* nmh_last_error(void);
/* "src=<hash of the sources the library was compiled from> arch=gfx950 fp_contract=off" */
NMH_API const char* nmh_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
