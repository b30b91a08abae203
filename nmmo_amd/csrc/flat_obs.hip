// flat_obs.hip — the pufferlib-flat float32 obs rows (23,987 per agent, SPEC.md §8) written
// incrementally into the handle's bound buffer (nmmo_obs_bind): a row stores only
// what differs from what the buffer already holds (ObsParams::zrow / zst). Replaces
// Env._compute_observations + pufferlib's flatten/pad (the rows the reference's learner decodes with
// unpack_batched_obs, baseline_policy.py:41) for the bound buffer, at every slot count; an unbound or
// untracked buffer gets every row in full from obs.hip's obs_kernel<kWrap>. The row-state protocol
// (kernels.h kZsZero / kZsExt / kZsTile, zs_pack) has this one reader and writer among the flat rows.
//
// Round 5 rewrite on agent_obs.h's pieces (the native kernel's staging, compaction and section bit
// fields). The round-4 flat kernel was issue-bound (per agent row 760 VALU, 524 SALU, 146 branch
// for 33 stores; profiles/r04/pmc_flat): one predicate per mask entry, index arithmetic per store,
// 31-way LDS bank conflicts on the Entity gathers and SGPR spills. Here, per agent wave:
//  - ActionTargets: 25 chunks of 64 entries; chunk c's 64-bit mask is the OR of the sections' bit
//    fields at compile-time shifts (the Buy.MarketItem part from one ballot per 64 listings), and
//    lane L stores bit L of it as 0.f / 1.f -- one v_cndmask on the SGPR pair
//    (__builtin_amdgcn_inverse_ballot_w64) and one store per chunk. Chunks holding only Buy entries
//    at or past the row's known-zero threshold are skipped. AgentId / CurrentTick ride in the last
//    chunk's lanes 50 and 51;
//  - the env's Entity columns staged with an odd dword stride (conflict-free lane-per-field reads),
//    the window compaction from packed datastore-row words held in registers, and the workgroup's
//    window rows and item words staged in LDS up front, so the agent loop issues no global load
//    (except a Task section to rewrite, once per task change, and the listings whose item words
//    did not fit LDS: none up to 256 listings);
//  - every store goes to the row's wave-uniform base (SGPRs) plus a per-lane constant offset.
#include "agent_obs.h"

namespace nmmo {

#ifndef NMMO_FO_ABL  // diagnostic ablation (timing attribution only, wrong rows): bit 1 masks, 2 Entity,
#define NMMO_FO_ABL 0  // 4 Inventory, 8 Market, 16 Tile, 32 compaction, 64 the agent loop (prologue only),
#endif                 // 128 everything (an empty launch), 256 rows aliased onto 128 per XCD (stores L2-resident)
                       // (tools/debug/variants.py; in the mirror variant bit 1 takes the mask pass out, and
                       // with it the row-state write-back: every row is then written as one of unknown state;
                       // bit 64 keeps the pass, prologue work, which then writes the state of rows nobody writes)
#ifndef NMMO_FO_STAMPS  // diagnostic: s_memtime per section of every alive row (tools/debug/fo_stamps.py)
#define NMMO_FO_STAMPS 0
#endif
#if NMMO_FO_STAMPS
constexpr int kFoStamps = 12;  // loop top, compaction, sections, chunks 0-1, Buy-only chunks, tail chunks,
                              // Entity, Inventory, Market, Task, Tile, state
__device__ uint64_t fo_stamp_buf[1 << 17][kFoStamps];
__device__ uint64_t fo_wave_buf[1 << 15][6];  // per wave: entry, staged, windows, loop start, loop end, env
#define FO_STAMP(k) fst[k] = __builtin_amdgcn_s_memtime()
#else
#define FO_STAMP(k) (void)0
#endif
#ifndef NMMO_FO_XCD  // (A/B knob: 1 = a 1-D grid with an env's groups on one XCD, agent_obs.h ao_env_group)
#define NMMO_FO_XCD 1
#endif
#ifndef NMMO_FO_TILE_SKIP  // (A/B knob: 1 = round 5's Tile component skip, tools/debug/variants.py)
#define NMMO_FO_TILE_SKIP 0
#endif
#ifndef NMMO_FO_TASK_BATCH  // (A/B knob: tools/debug/variants.py)
#define NMMO_FO_TASK_BATCH 8
#endif
constexpr int kFoTaskBatch = NMMO_FO_TASK_BATCH;  // Task floats per lane loaded before their stores
constexpr int kFoStagedListings = 64;   // listings whose item words are staged at the least (fo_staged)
constexpr int kFoChunks = 25;           // 64-entry chunks over the 1,586 mask entries (+ id, tick)
static_assert(kFoChunks * 64 >= kMaskN + 2 && (kFoChunks - 1) * 64 < kMaskN, "mask chunks");
// AgentId and CurrentTick ride in the last chunk right after the mask entries; chunks 2..16 hold
// only Buy.MarketItem entries (fo_slot)
static_assert(kFlatId == kMaskN && kFlatTick == kMaskN + 1 && kFlatEntity == kMaskN + 2, "id, tick in the last chunk");
static_assert(kWireBuyLo / 64 == 1 && (kWireBuyLo + NMMO_MARKET_ROWS) / 64 == 17, "Buy.MarketItem: chunks 1 to 17");
// (the flat row's section offsets are compile-time, obs_layout.h: every runtime offset was an SGPR
// the agent loop spilled)

// LDS: agent_obs.h's Entity columns T | the listings' pool | per-wave visible rows | the workgroup's
// staged window rows (16 B each, realigned) | its item words. 31,936 B at S = 384: 5 workgroups per
// CU (LDS is allocated in 1,280-B granules, so 5 fit up to 32,000 B, not 32,768).
// The listings' pool (2,560 B) is filled from both ends: price | owner << 8 (u16) of all nm listings
// upwards from its start, the item words of the first fo_staged(nm) listings downwards from its
// end -- every listing's up to nm = 256, 64 at nm = 1,024 (the pool's size: kFoStagedListings).
// Two more regions are shared by data that is never live together:
//  - the packed datastore-row words (pk, agent_obs.h) lie in the window rows' region: they are dead
//    once every lane holds its pr[] words, and the window rows are written after a barrier that
//    follows those loads (ao_stage_windows' before_writes);
//  - at S = 384 the item words lie in T's F_ROW and F_COL columns (adjacent, 1,544 B): after that
//    barrier nothing reads them -- an agent's own position is kept in a register (my_rc) and a
//    visible entity's comes from its packed word (ao_row / ao_col: the values the window test used).
//    A smaller S has smaller columns and LDS to spare: the item words follow the window rows.
// None of the regions' alignment depends on S: ao_stride(S) is twice an odd number for every S (383
// shares 384's), T is padded to 16 B, the pool, the visible rows and the window rows are multiples of
// 16 B, and fo_items_in_T takes the item words into T only where they land 8-B aligned.
constexpr int kFoVisw = (kNObs + 3) & ~3;            // visible-row words per wave (the compaction writes pos < kNObs)
constexpr int kFoWinRowBytes = 16, kFoWinAgentBytes = 15 * kFoWinRowBytes;
constexpr size_t kFoWinBytes = (size_t)kAoAgents * kFoWinAgentBytes, kFoItemBytes = (size_t)kAoAgents * kInv * 8;
static_assert(F_COL == F_ROW + 1 && kAoPkBytes <= kFoWinBytes, "shared LDS regions");
__host__ __device__ constexpr bool fo_items_in_T(int S) {
  return (size_t)2 * ao_stride(S) * 2 >= kFoItemBytes && (F_ROW * ao_stride(S) * 2) % 8 == 0;
}
constexpr int kFoListPool = NMMO_MARKET_ROWS * 2 + kFoStagedListings * 8;
// listings whose item words fit the pool beside nm price | owner entries (8-B aligned)
__host__ __device__ constexpr int fo_staged(int nm) {
  return nm < ((kFoListPool - ((2 * nm + 7) & ~7)) >> 3) ? nm : (kFoListPool - ((2 * nm + 7) & ~7)) >> 3;
}
static_assert(fo_staged(NMMO_MARKET_ROWS) == kFoStagedListings && fo_staged(256) == 256 && fo_staged(257) == 255 &&
                  fo_staged(0) == 0 && kFoListPool % 16 == 0, "listings' pool");
__host__ __device__ constexpr size_t fo_lds_bytes(int S) {
  return ao_columns_lds(S) + (size_t)kFoListPool +
         (size_t)kAoWaves * kFoVisw * 4 + kFoWinBytes + (fo_items_in_T(S) ? 0 : kFoItemBytes);
}
constexpr size_t kFoLdsGranule = 1280;  // gfx950's LDS allocation unit (tools/occupancy_probe.hip)
// (the product shape; an A/B build with another NMMO_AO_AGENTS keeps its item words after the window rows)
static_assert(kAoAgents != 16 ||
                  (5 * fo_lds_bytes(kMaxSlots) <= 160 * 1024 && fo_items_in_T(kMaxSlots) &&
                   5 * ((fo_lds_bytes(kMaxSlots) + kFoLdsGranule - 1) / kFoLdsGranule * kFoLdsGranule) <= 160 * 1024),
              "5 workgroups per CU");

// The mirror variant (kMirror: the obs launch of a step whose tick wrote DevState::fm, 384 slots): no
// staged columns and no pk. LDS: the workgroup's own agents' mirror rows [16][32] int16 | the first
// kFoGather visible entities' mirror rows of every agent [16][kFoGather][32] int16 | the listings'
// pool | every agent's visible rows [16][kFoVisw] | the window rows | the item words (a region of
// their own: nothing is aliased, so the windows need no barrier ahead of their writes).
// kFoGather: the smallest even count covering >= 99 % of the agent rows of the bench scenario
// (tools/flat_window_counts.py, DESIGN §3.2d: 99.7 % see at most 12 entities, 99.3 % at most 11);
// the rows past it take a global load each, in a loop of their own. A multiple of 4: a 16-B load
// instruction of a wave gathers 16 rows (4 lanes per 64-B row).
constexpr int kFoGather = 12;
static_assert(kFoGather % 4 == 0 && kFoGather <= 16 && kFoGather <= kNObs, "gathered rows");
constexpr size_t kFoOwnBytes = (size_t)kAoAgents * kMirrorCols * 2;
constexpr size_t kFoGatBytes = (size_t)kAoAgents * kFoGather * kMirrorCols * 2;
constexpr size_t kFoMirrorLds =
    kFoOwnBytes + kFoGatBytes + (size_t)kFoListPool + (size_t)kAoAgents * kFoVisw * 4 + kFoWinBytes + kFoItemBytes;
static_assert(5 * ((kFoMirrorLds + kFoLdsGranule - 1) / kFoLdsGranule * kFoLdsGranule) <= 160 * 1024 &&
                  kFoOwnBytes % 16 == 0 && kFoGatBytes % 16 == 0, "5 workgroups per CU");

// Low 64 bits of the 128-bit field (hi:lo) shifted left by kSh (right when negative): the part of a
// section whose bit 0 sits at chunk bit kSh.
template <int kSh>
__device__ __forceinline__ uint64_t fo_shift(uint64_t lo, uint64_t hi) {
  if constexpr (kSh >= 64) {
    return 0ull;
  } else if constexpr (kSh > 0) {
    return lo << kSh;
  } else if constexpr (kSh == 0) {
    return lo;
  } else if constexpr (-kSh < 64) {
    return (lo >> (-kSh)) | (hi << (64 + kSh));
  } else if constexpr (-kSh < 128) {
    return hi >> (-kSh - 64);
  } else {
    return 0ull;
  }
}
// Section k's contribution to chunk kC (entries 64 kC .. 64 kC + 63 of the flat mask part)
template <int kK, int kC>
__device__ __forceinline__ uint64_t fo_sec(uint64_t lo, uint64_t hi) {
  constexpr int off = sec_flat(kK), n = kSecN[kK];
  if constexpr (off >= 64 * kC + 64 || off + n <= 64 * kC) return 0ull;
  else return fo_shift<off - 64 * kC>(lo, hi);
}
// The 11 section fields (every section but Buy.MarketItem) in chunk kC
template <int kC>
__device__ __forceinline__ uint64_t fo_chunk(const AoSections& x) {
  return fo_sec<0, kC>(x.s0, 0ull) | fo_sec<1, kC>(x.s1[0], x.s1[1]) | fo_sec<3, kC>(x.s3, 0ull) |
         fo_sec<4, kC>(x.s4, 0ull) | fo_sec<5, kC>(x.s5[0], x.s5[1]) | fo_sec<6, kC>(x.s6[0], x.s6[1]) |
         fo_sec<7, kC>(x.s7[0], x.s7[1]) | fo_sec<8, kC>(x.s8, 0ull) | fo_sec<9, kC>(x.s9, 0ull) |
         fo_sec<10, kC>(x.s10[0], x.s10[1]) | fo_sec<11, kC>(x.s11, 0ull);
}
__device__ __forceinline__ float fo_bit(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m) ? 1.f : 0.f; }
// row[idx] = v as base + zero-extended 32-bit byte offset: the store's SGPR-base (saddr) form, one
// offset VGPR, instead of a sign-extended 64-bit address built per store (4 VALU each)
__device__ __forceinline__ void fo_st(float* row, uint32_t idx, float v) {
  *reinterpret_cast<float*>(reinterpret_cast<char*>(row) + (idx << 2)) = v;
}

// The row's tracked ActionTargets chunks (ObsParams::zext): chunks 0 and 1 (Style, Attack.Target,
// Buy's first 24 entries) and 17..24 (Buy's last 40 entries and no-op, then every other section,
// AgentId, CurrentTick) as slots 0..9. A chunk whose mask equals the one the row was last written
// with is not stored again: per tick an agent's Move and Attack.Target bits change, while the
// gold-, inventory- and same-tile-driven sections mostly do not.
constexpr int kFoTail0 = (kWireBuyLo + NMMO_MARKET_ROWS) / 64;  // 17
__host__ __device__ constexpr int fo_slot(int c) { return c < 2 ? c : c - kFoTail0 + 2; }
static_assert(fo_slot(kFoChunks - 1) == 9 && kZext == 10 + 1 + 12, "tracked chunks | position | items");
struct FoImg {
  bool ext;        // the row's extended state is valid (else every chunk is stored)
  uint32_t lo, hi; // the wave's loaded masks: lane 10 j + slot = agent j's chunk `slot`
  int j10;         // 10 j
  int nimg;        // the new masks: lane 2 slot / 2 slot + 1 = slot's lo / hi word
  int nst;         // mask entries (+ id, tick) stored
};
__device__ __forceinline__ uint64_t fo_prev(const FoImg& g, int slot) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)g.lo, g.j10 + slot) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)g.hi, g.j10 + slot) << 32;
}
// chunk kC with mask m: stored unless the row holds it already; its mask goes into the new image
template <int kC>
__device__ __forceinline__ void fo_put(float* row, FoImg& g, uint64_t m, float aid, float tick) {
  constexpr int sl = fo_slot(kC);
  const int lane = ao_lane();
  const bool same = g.ext && m == fo_prev(g, sl);
  if constexpr (kC == kFoChunks - 1) {  // + AgentId, CurrentTick right after the mask entries
    constexpr int n = kMaskN - 64 * kC;
    if (!same) {
      if (lane < n + 2) fo_st(row, 64 * kC + lane, lane < n ? fo_bit(m) : lane == n ? aid : tick);
      g.nst += n + 2;
    } else {
      if (lane == n + 1) fo_st(row, 64 * kC + lane, tick);  // the tick changes every step
      g.nst += 1;
    }
  } else if (!same) {
    fo_st(row, 64 * kC + lane, fo_bit(m));
    g.nst += 64;
  }
  g.nimg = writelane<2 * sl>((int)(uint32_t)m, g.nimg);
  g.nimg = writelane<2 * sl + 1>((int)(uint32_t)(m >> 32), g.nimg);
}
template <int kC>
__device__ __forceinline__ void fo_tail_chunks(float* row, FoImg& g, const AoSections& x, uint64_t buy17, float aid,
                                               float tick) {
  if constexpr (kC < kFoChunks) {
    uint64_t m = fo_chunk<kC>(x);
    if constexpr (kC == kFoTail0) m |= buy17 | 1ull << ((kWireBuyLo + NMMO_MARKET_ROWS) & 63);
    fo_put<kC>(row, g, m, aid, tick);
    fo_tail_chunks<kC + 1>(row, g, x, buy17, aid, tick);
  }
}

// The mirror variant's mask pass: the tracked chunks of all of a wave's agents built
// once per wave, lane 10 j + slot = agent j's chunk `slot` (the layout the extended state is loaded
// in), instead of once per row from wave-uniform values with 63 lanes idle.
//  - the section fields over the visible rows and the inventory come from ballots whose lane
//    16 j + k tests agent j's visible row / item k: four agents per ballot;
//  - lane 10 j + slot assembles its chunk from agent j's fields (fo_chunk on per-lane values);
//  - one compare with the loaded masks and one ballot give the changed bit of every (agent, chunk),
//    one compare of the item words the Inventory sections' (bit 12 j + k);
//  - the row state of the wave's agents in the realm goes out in a few wave-wide stores.
// kFoPassRows: the visible rows a lane group holds. An agent that sees more (0.004 % of the bench
// scenario's rows, tools/flat_window_counts.py) takes ao_sections' ballots over all of its rows, in
// a loop of its own, for the three fields they feed. The listings need no bound: Buy's words 0 and
// 15 (the tracked chunks' part) are one ballot per agent each, as in the per-row code.
constexpr int kFoPassRows = 16;
static_assert(kFoPassRows == 16 && kAoAgents / kAoWaves * kFoPassRows <= 64 && kInv <= kFoPassRows &&
                  kFoGather <= kFoPassRows, "a 16-lane group per agent");
constexpr int kFoBuyLane = 48;  // lane kFoBuyLane + j of FoPass::lo / hi: agent j's Buy word 0
struct FoPass {
  uint32_t lo, hi;  // lane 10 j + slot: agent j's new tracked mask; lanes 40 + j: as loaded (the Tile position)
  uint64_t chg;     // bit 10 j + slot: the row does not hold that mask
  uint64_t idiff;   // bit 12 j + k: the row's Inventory section was not written from item word k
};
template <int kSl>
__device__ __forceinline__ void fo_pass_chunks(const AoSections& x, int sl, uint64_t& m) {
  if constexpr (kSl < 10) {
    constexpr int c = kSl < 2 ? kSl : kSl - 2 + kFoTail0;
    static_assert(fo_slot(c) == kSl, "tracked chunk");
    const uint64_t mc = fo_chunk<c>(x);
    if (sl == kSl) m = mc;
    fo_pass_chunks<kSl + 1>(x, sl, m);
  }
}
// own: the workgroup's own agents' mirror rows; visw: the wave's agents' visible rows (agent j's at
// j * kFoVisw); my_*: lane j = agent abase + kAoWaves * j (my_alive 0 past P); zvalid / zextv: the
// agents' row state bits; img / pinv: the loaded extended state (zero where not valid)
template <bool kWrap>
__device__ __forceinline__ FoPass fo_mask_pass(const ObsParams& p, int e, int w, int abase, int nm, const int16_t* own,
                                               const uint32_t* visw, const uint8_t* wsb, const uint2* ist,
                                               const uint16_t* mpo, int my_nv, uint32_t my_rc, int my_prev, int my_alive,
                                               int my_task, uint64_t zvalid, uint64_t zextv, uint2 img, uint2 pinv) {
  constexpr int kPerWave = kAoAgents / kAoWaves;
  const bool combat = (p.systems & NMMO_SYS_COMBAT) != 0;
  const bool item = (p.systems & NMMO_SYS_ITEM) != 0;
  const bool exch = item && (p.systems & NMMO_SYS_EXCHANGE) != 0;
  const bool no_give = kWrap && (p.wflags & kWrapObsNoGive);
  const bool no_danger = kWrap && (p.wflags & kWrapObsNoDangerous);
  const int lane = lane_id(), P = p.P;
  // lane 16 j + k: agent j's visible row k (1 AttackTarget; 5 GiveTarget / 7 GoldTarget's same-tile
  // predicate) and its item k (3 Destroy / 4 GiveItem, 9 SellItem, 11 Use), as ao_sections
  const int gj = lane >> 4, gk = lane & 15, ga = abase + kAoWaves * gj, gla = w + kAoWaves * gj;
  const int grc = __shfl((int)my_rc, gj);
  const int gr = (int16_t)(grc & 0xFFFF), gc = grc >> 16;
  bool tgt = false, st = false;
  if (gk < __shfl(my_nv, gj)) ao_row_preds(visw[gj * kFoVisw + gk], ga, gr, gc, combat, no_danger, tgt, st);
  const uint64_t tb = __ballot(tgt), sb = __ballot(st);
  const uint2 it = gk < kInv ? ist[gla * kInv + gk] : make_uint2(0u, 0u);
  const uint64_t occ = __ballot(gk < kInv && it_type(it) != 0);
  const bool have = gk < __builtin_ctz(~((uint32_t)(occ >> (16 * gj)) & 0xFFFFu));  // the occupied prefix
  const uint64_t bfr = __ballot(have && !it_equipped(it) && !it_price(it));
  const uint64_t bse = __ballot(have && !it_equipped(it));
  uint64_t bus;
  {  // ao_usable_ballot, the level lookup within the lane group
    const int16_t* lvs = own + gla * kMirrorCols + F_MELEE_LEVEL;
    int lv = 0;
    if (gk < 8) lv = lvs[2 * gk];
    else if (gk == 8) lv = max((int)lvs[0], max((int)lvs[F_RANGE_LEVEL - F_MELEE_LEVEL], (int)lvs[F_MAGE_LEVEL - F_MELEE_LEVEL]));
    const int req = __shfl(lv, 16 * gj + ao_req_lane(it_type(it)));
    bus = __ballot(ao_usable(it, have, req));
  }
  // lane 10 j + slot: agent j's fields (the lanes from 40 on compute agent 3's again, unused)
  const int ja = min(lane / 10, kPerWave - 1), sl = lane - 10 * (lane / 10), la = w + kAoWaves * ja;
  const uint64_t noop = 1ull << (kNObs - 64);
  uint64_t t0 = (uint32_t)(tb >> (16 * ja)) & 0xFFFFu, t1 = 0ull, s0 = (uint32_t)(sb >> (16 * ja)) & 0xFFFFu, s1 = 0ull;
#pragma unroll 1
  for (int j = 0; j < kPerWave; j++) {  // an agent past the lane group: ao_sections' ballots over all of its rows
    const int nv = __builtin_amdgcn_readlane(my_nv, j);
    if (nv <= kFoPassRows) continue;
    const int rcj = __builtin_amdgcn_readlane((int)my_rc, j), a = abase + kAoWaves * j;
    const int r = (int16_t)(rcj & 0xFFFF), c = rcj >> 16;
    uint64_t tj[2] = {0ull, 0ull}, sj[2] = {0ull, 0ull};
#pragma unroll
    for (int h = 0; h < 2; h++) {
      if (64 * h >= nv) break;
      const int k = 64 * h + lane;
      bool tg = false, sm = false;
      if (k < nv) ao_row_preds(visw[j * kFoVisw + k], a, r, c, combat, no_danger, tg, sm);
      tj[h] = __ballot(tg);
      sj[h] = __ballot(sm);
    }
    if (ja == j) t0 = tj[0], t1 = tj[1], s0 = sj[0], s1 = sj[1];
  }
  AoSections x;
  x.s1[0] = t0;
  x.s1[1] = t1 | noop;
  x.s5[0] = item && !no_give ? s0 : 0ull;
  x.s5[1] = (item && !no_give ? s1 : 0ull) | noop;
  x.s7[0] = exch && !no_give ? s0 : 0ull;
  x.s7[1] = (exch && !no_give ? s1 : 0ull) | noop;
  const uint64_t ifr = (uint32_t)(bfr >> (16 * ja)) & 0xFFFFu;
  x.s3 = (item ? ifr : 0ull) | 1ull << kInv;
  x.s4 = (item && !no_give ? ifr : 0ull) | 1ull << kInv;
  x.s9 = (exch ? (uint64_t)((uint32_t)(bse >> (16 * ja)) & 0xFFFFu) : 0ull) | 1ull << kInv;
  x.s11 = (item ? (uint64_t)((uint32_t)(bus >> (16 * ja)) & 0xFFFFu) : 0ull) | 1ull << kInv;
  x.s0 = combat ? low_bits(kSecN[0]) : 0ull;
  x.s6[0] = x.s6[1] = x.s10[0] = x.s10[1] = 0ull;
  if (exch) {
    const int gold = own[la * kMirrorCols + F_GOLD];
    const int ng = no_give ? min(gold, 1) : min(gold, kSecN[6]);
    x.s6[0] = low_bits(ng);
    x.s6[1] = low_bits(ng - 64);
    x.s10[0] = low_bits(kSecN[10]);
    x.s10[1] = low_bits(kSecN[10] - 64);
    if constexpr (kWrap) {
      const int pp = __shfl(my_prev, ja);
      if ((p.wflags & kWrapObsPrice) && pp >= 0 && pp < kSecN[10]) {
        const uint64_t clr = ~(1ull << (pp & 63));
        if (pp < 64) x.s10[0] &= clr;
        else x.s10[1] &= clr;
      }
    }
  }
  {  // 8 Move: ao_move_bits from the staged window rows
    const uint8_t* wa = wsb + la * kFoWinAgentBytes;
    uint32_t b = 0u;
#pragma unroll
    for (int d = 0; d < 5; d++)
      if (!impassable((int)wa[(kVision + dir_dr(d)) * kFoWinRowBytes + kVision + dir_dc(d)])) b |= 1u << d;
    x.s8 = b;
  }
  uint64_t m = 0ull;
  fo_pass_chunks<0>(x, sl, m);
  // Buy.MarketItem in the tracked chunks: word 0 (listings 0..63) in chunk 1, word 15 (listings from
  // 960) in chunk 17 with the no-op bit; one ballot per agent over lane = listing
  uint64_t bw0 = 0ull, bw15 = 0ull;
  FoPass o;
  o.lo = img.x;
  o.hi = img.y;
  if (exch && nm > 0) {
    const uint32_t po0 = lane < nm ? mpo[lane] : 0u, po15 = 15 * 64 + lane < nm ? mpo[15 * 64 + lane] : 0u;
#pragma unroll
    for (int j = 0; j < kPerWave; j++) {
      const int a = abase + kAoWaves * j;
      const int gold = __builtin_amdgcn_readfirstlane((int)own[(w + kAoWaves * j) * kMirrorCols + F_GOLD]);
      const uint64_t b0 = __ballot(lane < nm && (int)(po0 & 255u) <= gold && (int)(po0 >> 8) != a);
      uint64_t b15 = 0ull;
      if (nm > 15 * 64) b15 = __ballot(15 * 64 + lane < nm && (int)(po15 & 255u) <= gold && (int)(po15 >> 8) != a);
      if (ja == j) bw0 = b0, bw15 = b15;
      if (lane == kFoBuyLane + j) o.lo = (uint32_t)b0, o.hi = (uint32_t)(b0 >> 32);  // (else zero, as loaded)
    }
  }
  if (sl == 1) m |= bw0 << (kWireBuyLo & 63);
  if (sl == 2) m |= bw15 >> (64 - (kWireBuyLo & 63)) | 1ull << ((kWireBuyLo + NMMO_MARKET_ROWS) & 63);
  // compare with what the rows hold; the new masks take the loaded ones' place
  const bool ext = (zextv >> ja) & 1;
  o.chg = __ballot(lane < 10 * kPerWave && (!ext || (uint32_t)m != img.x || (uint32_t)(m >> 32) != img.y));
  if (lane < 10 * kPerWave) o.lo = (uint32_t)m, o.hi = (uint32_t)(m >> 32);
  const int ji = min(lane / kInv, kPerWave - 1);
  const uint2 iw = ist[(w + kAoWaves * ji) * kInv + lane % kInv];
  const bool idl = lane < kInv * kPerWave && (!((zextv >> ji) & 1) || iw.x != pinv.x || iw.y != pinv.y);
  o.idiff = __ballot(idl);
  // the row state of the agents in the realm (a dead row's paths write their own): the masks and
  // the position, the item words that changed, the tag and the state word
  {
    const int jp = lane < 10 * kPerWave ? ja : min(lane - 10 * kPerWave, kPerWave - 1);
    const size_t ai = (size_t)e * P + min(abase + kAoWaves * jp, P - 1);
    uint2 wv = make_uint2(o.lo, o.hi);
    const int rcp = __shfl((int)my_rc, jp);  // (every lane, as ali below)
    if (lane >= 10 * kPerWave) {
      wv = make_uint2((uint32_t)((int)(int16_t)(rcp & 0xFFFF) | (rcp >> 16) << 8), 0u);
    }
    const int alp = __shfl(my_alive, jp);
    if (lane < 11 * kPerWave && alp) reinterpret_cast<uint2*>(p.zext)[ai * kZext + (lane < 10 * kPerWave ? sl : 10)] = wv;
    const size_t ii = (size_t)e * P + min(abase + kAoWaves * ji, P - 1);
    const int ali = __shfl(my_alive, ji);  // (every lane: a cross-lane read under idl would miss lanes 0..3)
    if (idl && ali) reinterpret_cast<uint2*>(p.zext)[ii * kZext + 11 + lane % kInv] = iw;
    if (lane < kPerWave && my_alive) {
      const size_t am = (size_t)e * P + abase + kAoWaves * lane;
      if (!((zvalid >> lane) & 1)) p.zrow[am] = p.ztag;
      p.zst[am] = zs_pack((my_nv + 1) & ~1, nm, my_task) | kZsExt;
    }
  }
  return o;
}

// item_col (common.h) for a column fixed per lane (Inventory / Market chunks: lane L holds
// column L % 16 of every item it writes): a per-lane descriptor built once, so an entry is one
// bit-field extract plus a type-mask term instead of a 16-way select per entry.
//   value = bfe(x or y, sh, wd) + own * owner + mult * level + (mult ? b : 0),
//   mult = bit(type) of tmA * aA + bit(type) of tmB * aB
struct IcDesc {
  uint32_t tmA, tmB;
  uint32_t f;  // sel | sh << 1 | wd << 6 | own << 11 | aA << 12 | aB << 16 | b << 20
};
__device__ __forceinline__ IcDesc ic_desc(int col) {
  auto bits = [](int lo, int hi) { return ((2u << hi) - 1u) & ~((1u << lo) - 1u); };
  IcDesc d{0u, 0u, 0u};
  auto bf = [&](int sel, int sh, int wd) { d.f = (uint32_t)(sel | sh << 1 | wd << 6); };
  switch (col) {
    case 0: bf(1, 16, 16); break;  // row
    case 1: bf(0, 0, 5); break;    // type
    case 2: d.f = 1u << 11; break; // owner
    case 3: bf(0, 5, 4); break;    // level
    case 5: bf(1, 0, 16); break;   // quantity
    case 6: case 7: case 8:        // melee / range / mage attack
      d.tmA = 1u << (T_SPEAR + col - 6) | 1u << (T_WHETSTONE + col - 6);
      d.f = 5u << 12 | 5u << 20;
      break;
    case 9: case 10: case 11:      // defense
      d.tmA = bits(T_HAT, T_BOTTOM);
      d.tmB = bits(T_ROD, T_CHISEL);
      d.f = 3u << 12 | 2u << 16;
      break;
    case 12: d.tmA = 1u << T_POTION; d.f = 5u << 12 | 50u << 20; break;
    case 13: d.tmA = 1u << T_RATION; d.f = 5u << 12 | 50u << 20; break;
    case 14: bf(0, 9, 1); break;   // equipped
    case 15: bf(0, 10, 7); break;  // listed price
    default: break;                // 4: zero
  }
  return d;
}
__device__ __forceinline__ float ic_value(uint2 w, int owner, const IcDesc& d) {
  const int type = (int)(w.x & 31u), lvl = (int)((w.x >> 5) & 15u);
  const uint32_t bfv = __builtin_amdgcn_ubfe((d.f & 1u) ? w.y : w.x, (d.f >> 1) & 31u, (d.f >> 6) & 31u);
  const int ta = (int)((d.tmA >> type) & 1u), tb = (int)((d.tmB >> type) & 1u);
  const int mult = ta * (int)((d.f >> 12) & 15u) + tb * (int)((d.f >> 16) & 15u);
  return (float)((int)bfv + (int)((d.f >> 11) & 1u) * owner + mult * lvl + ((ta | tb) ? (int)(d.f >> 20) : 0));
}
static_assert(T_POTION < 32 && T_RATION < 32 && T_WHETSTONE + 2 < 32, "item type masks");

// Window compaction as agent_obs.h's ao_compact over all kAoRows register words (the rows past S
// hold kAoEmpty, outside every window): no bound on S to keep live across the agent loop
__device__ __forceinline__ int fo_compact(const uint32_t (&pr)[kAoRows], int r, int c, uint32_t* visw) {
  int nvis = 0;
  const uint32_t rc = (uint32_t)r | (uint32_t)c << 16;
#pragma unroll
  for (int i = 0; i < kAoRows; i++) {
    const bool in = ao_in_window(pr[i], rc);
    const uint64_t b = __ballot(in);
    const int pos = nvis + __popcll(b & lanes_below());
    if (in && pos < kNObs) visw[pos] = pr[i];
    nvis += __popcll(b);
  }
  return nvis;
}

typedef const __attribute__((address_space(4))) ObsParams* FoArgs;  // the kernel's argument segment

// kS: the slot count when known at compile time (C3 / C4: 128 players + 256 NPCs), 0 = p.S. With
// it the staged-column offsets are immediates instead of uniform values the agent loop keeps live.
// 5 waves per SIMD (5 workgroups of 4 waves per CU): 96 VGPRs, which the kernel fits without scratch.
// kAligned: S % 8 == 0 (agent_obs.h's 16-B column loads); false stages any S element by element.
// kMirror: p.fpk / p.frows hold the tick's entity mirror of this very state (kernels.h): the packed
// row words come from p.fpk, the workgroup's own agents' rows and its agents' first kFoGather
// visible rows from p.frows, and nothing is staged (kFoGather above).
template <bool kWrap, int kS, bool kAligned = true, bool kMirror = false>
__global__ void __launch_bounds__(64 * kAoWaves) __attribute__((amdgpu_waves_per_eu(5, 5))) flat_obs_kernel(ObsParams p) {
  static_assert(!kMirror || (kS == kMaxSlots && kAligned), "the mirror variant: 384 slots");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int S = kS ? kS : p.S, P = p.P, Sp = ao_stride(S), tdim = p.task_dim, elems = kFlatTask + tdim + kTileN;
  constexpr int kPerWave = kAoAgents / kAoWaves;
  static_assert(!kMirror || (kPerWave * kFoGather) % 16 == 0, "gather: 16 rows per load instruction");
  int16_t* T = reinterpret_cast<int16_t*>(smem);  // kMirror: own, the workgroup's own agents' mirror rows
  int16_t* gat = reinterpret_cast<int16_t*>(smem + kFoOwnBytes);               // kMirror: the gathered rows
  uint16_t* mpo = reinterpret_cast<uint16_t*>(smem + (kMirror ? kFoOwnBytes + kFoGatBytes : ao_columns_lds(S)));  // [1024] price | owner << 8
  uint32_t* visw_all = reinterpret_cast<uint32_t*>(mpo) + kFoListPool / 4;       // [4][100] (kMirror: [16][100])
  uint2* mtop = reinterpret_cast<uint2*>(visw_all) - 1;  // mtop[-k]: listing k's item word (k < fo_staged(nm))
  uint32_t* wst = visw_all + (kMirror ? kAoAgents : kAoWaves) * kFoVisw;        // [16][15][4] window rows
  uint32_t* pk = wst;  // the packed datastore rows, until the window rows are written (fo_lds_bytes)
  uint2* ist = reinterpret_cast<uint2*>(!kMirror && fo_items_in_T(S) ? smem + (size_t)F_ROW * Sp * 2   // [16][12] item words
                                                                     : reinterpret_cast<unsigned char*>(wst) + kFoWinBytes);
#if NMMO_FO_XCD  // 1-D grid, an env's groups back to back on one XCD (agent_obs.h ao_env_group)
  int el, g;
  ao_env_group(p.env_list ? p.n_list : p.n_envs, (p.P + kAoAgents - 1) / kAoAgents, el, g);
#else
  const int el = blockIdx.x, g = blockIdx.y;
#endif
  const int e = p.env_list ? p.env_list[el] : el, tid = threadIdx.x, lane = lane_id();
  if ((unsigned)e >= (unsigned)p.n_envs) return;  // a bad list id (the tick records it)
  if (NMMO_FO_ABL & 128) return;
#if NMMO_FO_STAMPS
  uint64_t wst_[6];
  wst_[0] = __builtin_amdgcn_s_memtime();
#endif
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  // The prologue in two memory round trips: (1) the stage's loads, the listings' count and mlist
  // words and this wave's agents' words; (2) after the stage's LDS writes, the listed items, the
  // agents' extended row state and the workgroup's windows. (Issued where each was first needed,
  // the count -> mlist -> item chain, the stage, the windows and the extended state were six.)
  // (kMirror: trip 1 loads the packed row words, the own agents' mirror rows and the positions
  // instead of the stage's columns, and the windows of trip 2 follow the compaction, which runs for
  // all of the wave's agents between the trips; trip 2 also gathers their visible rows)
  AoStage sg;
  const int16_t* M = kMirror ? p.frows + (size_t)e * S * kMirrorCols : nullptr;  // the env's mirror rows
  uint32_t pr[kAoRows];  // this lane's datastore rows 1 + lane + 64 i
  uint4 ow = make_uint4(0u, 0u, 0u, 0u);
  int wpr = 0, wpc = 0;  // kMirror: the window thread's agent's position
  if constexpr (kMirror) {
    sg.nm = p.mcount[e];
    sg.mv = p.mlist[(size_t)e * NMMO_MARKET_ROWS + min(tid, NMMO_MARKET_ROWS - 1)];
#pragma unroll
    for (int i = 0; i < kAoRows; i++) pr[i] = p.fpk[(size_t)e * kMaxSlots + lane + 64 * i];
    // (every wave loads the 1 KB, wave 0 writes it: no branch around a load)
    ow = reinterpret_cast<const uint4*>(M + (size_t)min(g * kAoAgents + ((tid >> 2) & (kAoAgents - 1)), P - 1) * kMirrorCols)[tid & 3];
    const int16_t* wr = M + (size_t)min(g * kAoAgents + tid / 15, P - 1) * kMirrorCols;
    wpr = wr[F_ROW];
    wpc = wr[F_COL];
  } else {
    ao_stage_load<kAligned>(p, e, sg);
  }
  const int16_t* E = p.ent + (size_t)e * NMMO_NF * S;
  const int abase = g * kAoAgents + w;
  int my_task = 0, my_prev = -1, my_alive = 0;  // lane j: agent abase + 4 j
  uint64_t my_z = 0, my_s = 0;                  // its row state tag and word
  const bool mine = lane < kPerWave && abase + kAoWaves * lane < P;
  {  // every lane loads (a clamped agent), the values kept for its own agent below
    const int aj = min(abase + kAoWaves * min(lane, kPerWave - 1), P - 1);
    const size_t ai = (size_t)e * P + aj;
    my_task = p.assign[ai];
    my_alive = kMirror ? M[(size_t)aj * kMirrorCols + kMirrorCols - 1] : E[F_ALIVE * S + aj];
    if (p.zrow) {
      my_z = p.zrow[ai];
      my_s = p.zst[ai];
    }
    if constexpr (kWrap)
      if (p.ws) my_prev = p.ws[ai].prev_price;
  }
  uint32_t my_rc;  // its position, row | col << 16 (T's row / column columns are reused below)
  if constexpr (kMirror) {
    const int16_t* mr = M + (size_t)min(abase + kAoWaves * min(lane, kPerWave - 1), P - 1) * kMirrorCols;
    my_rc = (uint32_t)(uint16_t)mr[F_ROW] | (uint32_t)(uint16_t)mr[F_COL] << 16;
    if (tid < kAoAgents * 4) reinterpret_cast<uint4*>(T)[tid] = ow;  // own[la][32], la = tid / 4
  } else {
    ao_stage_store<kAligned>(p, e, T, pk, sg);
  }
  if (!mine) {
    my_task = 0, my_prev = -1, my_alive = 0;
    my_z = my_s = 0;
  }
  if constexpr (!kMirror) {
    const int aj = min(abase + kAoWaves * min(lane, kPerWave - 1), P - 1);
    my_rc = (uint32_t)(uint16_t)T[F_ROW * Sp + aj] | (uint32_t)(uint16_t)T[F_COL * Sp + aj] << 16;
  }
#if NMMO_FO_STAMPS
  wst_[1] = __builtin_amdgcn_s_memtime();
#endif

  if constexpr (!kMirror) {
#pragma unroll
    for (int i = 0; i < kAoRows; i++) pr[i] = pk[lane + 64 * i];
  }
  uint32_t* visw = visw_all + w * (kMirror ? kPerWave : 1) * kFoVisw;  // kMirror: agent j's at visw + j * kFoVisw
  // kMirror: the window compaction of all of the wave's agents in the realm, from pr[] (dead after
  // it), then the loads of their first kFoGather visible rows: 4 lanes per 64-B row, row t =
  // lane / 4 + 16 i of the wave's kPerWave * kFoGather (agent t / kFoGather's visible row
  // t % kFoGather; a row past its count loads the env's slot 0 and is never read)
  int my_nv = 0;  // lane j: agent j's visible count (capped at kNObs)
  constexpr int kGatIt = kPerWave * kFoGather / 16;
  static_assert(kGatIt >= 1 && kGatIt <= 4, "gather loads");
  uint4 gq0, gq1, gq2, gq3;  // (no array: one indexed from the listings' lambda went to scratch)
  gq0 = gq1 = gq2 = gq3 = make_uint4(0u, 0u, 0u, 0u);
  if constexpr (kMirror) {
#pragma unroll
    for (int j = 0; j < kPerWave; j++) {
      int nvj = 0;
      if (__builtin_amdgcn_readlane(my_alive, j) && !(NMMO_FO_ABL & 32)) {
        const int rcj = __builtin_amdgcn_readlane((int)my_rc, j);
        nvj = min(fo_compact(pr, (int16_t)(rcj & 0xFFFF), rcj >> 16, visw + j * kFoVisw), kNObs);
      }
      if (lane == j) my_nv = nvj;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    auto gather = [&](int i) {
      const int t = (lane >> 2) + 16 * i, tj = t / kFoGather, tk = t - tj * kFoGather;
      const uint32_t vw = visw[tj * kFoVisw + tk];
      const int slot = tk < __shfl(my_nv, tj) ? ao_slot(vw) : 0;
      return reinterpret_cast<const uint4*>(M + (size_t)min(slot, S - 1) * kMirrorCols)[lane & 3];
    };
    gq0 = gather(0);
    if constexpr (kGatIt > 1) gq1 = gather(1);
    if constexpr (kGatIt > 2) gq2 = gather(2);
    if constexpr (kGatIt > 3) gq3 = gather(3);
  }
  const uint8_t* wsb = reinterpret_cast<const uint8_t*>(wst);
  const float tickf = (float)p.env[(size_t)e * NMMO_NE + E_TICK];
  const bool exch = (p.systems & NMMO_SYS_ITEM) && (p.systems & NMMO_SYS_EXCHANGE);

  // bit j: agent j's row state describes this buffer / the row is all-zero / its Task section holds
  // its task's embedding / its extended state is valid; my_h = hv | hm << 12: its Entity rows >= hv
  // and its Market rows and Buy entries >= hm are zero (a row of unknown content: nothing known zero)
  const bool zvl = p.ztag && my_z == p.ztag;
  const bool zzl = zvl && (my_s & kZsZero);
  const uint64_t zvalid = __ballot(zvl), zzero = __ballot(zzl), ztask = __ballot(zvl && !zzl && zs_task(my_s) == my_task);
  const uint64_t zextv = __ballot(zvl && !zzl && (my_s & kZsExt));
  const uint64_t ztile = __ballot(zvl && (my_s & kZsTile));  // its Tile section was written by a consumer
  // the extended state (ObsParams::zext): lane 10 j + slot = agent j's tracked chunk `slot`, lane
  // 40 + j its Tile position; lane 12 j + k (inv) its item word k
  // (loaded by every lane from a valid address, with the listings' items and ahead of the
  // windows, and kept only where the state is valid)
  uint2 img = make_uint2(0u, 0u), pinv = make_uint2(0u, 0u);
  const int ja = lane < 40 ? lane / 10 : lane - 40, ji = lane / 12;
  const bool img_ok = lane < 44 && abase + kAoWaves * ja < P && ((zextv >> ja) & 1);
  const bool pinv_ok = lane < 48 && abase + kAoWaves * ji < P && ((zextv >> ji) & 1);
  if (kMirror || p.zext) {  // (kMirror: never NULL, launch_flat_obs; no branch around trip 2's loads)
    const int aa = min(abase + kAoWaves * min(ja, kPerWave - 1), P - 1);
    const int ai = min(abase + kAoWaves * min(ji, kPerWave - 1), P - 1);
    img = reinterpret_cast<const uint2*>(p.zext)[((size_t)e * P + aa) * kZext + (lane < 40 ? lane % 10 : 10)];
    pinv = reinterpret_cast<const uint2*>(p.zext)[((size_t)e * P + ai) * kZext + 11 + min(lane, 47) % 12];
  }
  const int nm = min(max(sg.nm, 0), NMMO_MARKET_ROWS), nst = fo_staged(nm);
  const uint2 lwd = ao_listing_load(p, e, sg);
  // the listings (ascending row) into LDS ahead of the windows' barrier, which publishes them.
  // The window rows overwrite pk, and at S = 384 the item words overwrite T's row / column columns:
  // a barrier after every wave's pr / my_rc loads and the windows' own position reads, ahead of those writes
  auto listings = [&]() {
    if constexpr (kMirror) {  // the gathered rows [w * kPerWave + j][k][32] beside the listings
      uint4* gd = reinterpret_cast<uint4*>(gat) + w * kGatIt * 64 + lane;
      gd[0] = gq0;
      if constexpr (kGatIt > 1) gd[64] = gq1;
      if constexpr (kGatIt > 2) gd[128] = gq2;
      if constexpr (kGatIt > 3) gd[192] = gq3;
    }
    if (tid < nm) {
      mpo[tid] = (uint16_t)(it_price(lwd) | ((sg.mv >> 16) & 255) << 8);
      if (tid < nst) mtop[-tid] = lwd;
    }
    for (int j = tid + (int)blockDim.x; j < nm; j += blockDim.x) {  // (more listings than threads)
      const int v = p.mlist[(size_t)e * NMMO_MARKET_ROWS + j];
      const int own = (v >> 16) & 255, slot = (v >> 24) & 15;
      const uint2 wd = p.items[((size_t)e * P + own) * kInv + slot];
      mpo[j] = (uint16_t)(it_price(wd) | own << 8);
      if (j < nst) mtop[-j] = wd;
    }
  };
  if constexpr (kMirror)  // (no region is aliased: no barrier ahead of the writes)
    ao_stage_windows_at<kAoAgents, kFoWinRowBytes / 4, true>(p, e, g, wpr, wpc, wst, ist, listings);
  else
    ao_stage_windows<kAoAgents, kFoWinRowBytes / 4>(p, e, g, T, Sp, wst, ist, listings, []() { __syncthreads(); });
#if NMMO_FO_STAMPS
  wst_[2] = __builtin_amdgcn_s_memtime();
#endif
  // Every prologue load has been waited on (the windows' LDS writes): a first use of img / pinv /
  // my_prev inside the agent loop (under a branch the waitcnt pass cannot see through) waited for
  // every store the row had issued -- one full drain per tracked chunk.
  asm volatile("" : "+v"(img.x), "+v"(img.y), "+v"(pinv.x), "+v"(pinv.y), "+v"(my_prev));
  if (!img_ok) img = make_uint2(0u, 0u);
  if (!pinv_ok) pinv = make_uint2(0u, 0u);
  const int my_h = !zvl ? (kNObs | NMMO_MARKET_ROWS << 12) : zzl ? 0 : (zs_hv(my_s) | zs_hm(my_s) << 12);
  // kMirror: every input of all of the wave's agents' masks is in LDS or registers here
  FoPass mp{img.x, img.y, ~0ull, ~0ull};
  if constexpr (kMirror) {
    if (!(NMMO_FO_ABL & 1))
      mp = fo_mask_pass<kWrap>(p, e, w, abase, nm, T, visw, wsb, ist, mpo, my_nv, my_rc, my_prev, my_alive, my_task, zvalid,
                               zextv, img, pinv);
  }
  int nrows = 0;                 // rows this wave wrote (rows_out[0])
  unsigned long long nbytes = 0;  // bytes this wave stored (rows_out[1])
  int wo[2];
  ao_win_offsets<kFoWinRowBytes>(wo);
  int toff[4];  // window tile lane + 64 i: (row offset) & 255 | (col offset) << 8
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int t = lane + 64 * i;
    toff[i] = ((t / 15 - kVision) & 255) | (t % 15 - kVision) * 256;
  }
  const int ef = lane & 31, eh = lane >> 5;  // Entity: field, row of the pair
  const int iq = lane >> 4;                  // Inventory: item of the chunk
  const IcDesc icd = ic_desc(lane & 15);      // Inventory / Market: column lane % 16

#if NMMO_FO_STAMPS
  wst_[3] = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll 1
  for (int j = 0; j < ((NMMO_FO_ABL & 64) ? 0 : kPerWave); j++) {
    const int a = abase + kAoWaves * j;
    if (a >= P) break;
    const int lane = ao_lane();  // (per iteration: lane predicates are not hoisted and spilled)
    // the kernel arguments the row's stores use, read from the argument segment per agent (scalar
    // loads) instead of held in SGPRs across the loop, which spilled them
    FoArgs kp = (FoArgs)__builtin_amdgcn_kernarg_segment_ptr();  // p is the only argument
    asm volatile("" : "+s"(kp));
    // the row pointer opaque per agent (its global address space kept), so the section bases are
    // computed from it in the loop instead of hoisted out of it (and spilled)
    auto grow = (__attribute__((address_space(1))) float*)(p.obs + ((NMMO_FO_ABL & 256)
        ? (size_t)(((e * P + a) & 15) + 16 * (blockIdx.x & 7)) : (size_t)e * P + a) * elems);
    asm volatile("" : "+s"(grow));
    float* row = (float*)grow;
    const bool zv = (zvalid >> j) & 1;
    const int hj = __builtin_amdgcn_readlane(my_h, j);
    const int hv = hj & 4095, hm = hj >> 12;
    if (!__builtin_amdgcn_readlane(my_alive, j)) {  // not in the realm: an all-zero row
      if ((zzero >> j) & 1) {  // zeroed by an earlier launch into this buffer
        if ((ztile >> j) & 1) {  // ... but a consumer wrote into its Tile section since
          wave_zero(row, kFlatTask + tdim, elems);
          nbytes += 4ull * (elems - kFlatTask - tdim);
          if (lane == 0) kp->zst[(size_t)e * P + a] = kZsZero;
          nrows++;
        }
        continue;
      }
      if (zv) {  // zero what the last write left nonzero
        wave_zero(row, 0, kFlatEntity + hv * NMMO_N_ENTITY_COLS);
        wave_zero(row, kFlatInv, kFlatMarket + hm * 16);
        wave_zero(row, kFlatTask, elems);
        nbytes += 4ull * (kFlatEntity + hv * NMMO_N_ENTITY_COLS + kFlatMarket + hm * 16 - kFlatInv + elems - kFlatTask);
      } else {
        wave_zero(row, 0, elems);
        nbytes += 4ull * elems;
      }
      if (lane == 0) {
        kp->zrow[(size_t)e * P + a] = kp->ztag;
        kp->zst[(size_t)e * P + a] = kZsZero;
      }
      nrows++;
      continue;
    }
    nrows++;
#if NMMO_FO_STAMPS
    uint64_t fst[kFoStamps];
#endif
    FO_STAMP(0);
    const int la = a - g * kAoAgents;
    const int rcj = __builtin_amdgcn_readlane((int)my_rc, j);
    const int r = (int16_t)(rcj & 0xFFFF), c = rcj >> 16;
    // the agent's own columns: T[f * Spa + tia] (kMirror: its row of the own tile, fields adjacent)
    const int16_t* Ta = kMirror ? T + la * kMirrorCols : T;
    const int Spa = kMirror ? 1 : Sp, tia = kMirror ? 0 : a;
    if constexpr (kMirror) visw = visw_all + (w * kPerWave + j) * kFoVisw;
    const int gold = __builtin_amdgcn_readfirstlane(Ta[F_GOLD * Spa + tia]);
    const int aid = __builtin_amdgcn_readfirstlane(Ta[F_ID * Spa + tia]);
    const uint8_t* wa = wsb + la * kFoWinAgentBytes;  // (rows realigned while staging: no column term)
    uint32_t wm[4];
#pragma unroll
    for (int i = 0; i < 4; i++) wm[i] = lane + 64 * i < 225 ? wa[ao_win_off(wo, i)] : 0u;
    // (kMirror: the mask pass has read the item words and the Move tiles; the Inventory section
    // reads the items when it is written)
    uint2 it = make_uint2(0u, 0u);
    uint32_t mv = 0u;
    int ninv = 0;  // occupied prefix
    if constexpr (!kMirror) {
      it = lane < kInv ? ist[la * kInv + lane] : make_uint2(0u, 0u);
      mv = ao_move_bits(wm[1]);
      ninv = __builtin_ctzll(~__ballot(lane < kInv && it_type(it) != 0));
    }
    int nv;
    if constexpr (kMirror) {  // compacted in the prologue
      nv = __builtin_amdgcn_readlane(my_nv, j);
    } else {
      nv = (NMMO_FO_ABL & 32) ? 0 : min(fo_compact(pr, r, c, visw), kNObs);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    FO_STAMP(1);
    const bool ext = (zextv >> j) & 1;  // the row's extended state is valid
    FoImg fg{ext, img.x, img.y, 10 * j, 0, 0};
    // ActionTargets (+ AgentId, CurrentTick)
    if constexpr (kMirror) {
      // the tracked chunks the row does not hold, from the mask pass's lanes: two v_readlane, the
      // lane's bit, one store each
      if (!(NMMO_FO_ABL & 1)) {
        const uint32_t chg = (uint32_t)(mp.chg >> (10 * j)) & 0x3FFu;
        auto pm = [&](int l) {
          return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mp.lo, l) |
                 (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mp.hi, l) << 32;
        };
        int nst = 0;
        FO_STAMP(2);
#pragma unroll 1
        for (uint32_t cs = chg & 3u; cs; cs &= cs - 1u) {  // chunks 0 and 1
          const int s = __builtin_ctz(cs);
          fo_st(row, 64 * s + lane, fo_bit(pm(10 * j + s)));
          nst += 64;
        }
        FO_STAMP(3);
        auto buy_word = [&](int m) {  // as below
          const int k = 64 * m + lane;
          bool bv = false;
          if (exch && k < nm) {
            const uint32_t po = mpo[k];
            bv = (int)(po & 255u) <= gold && (int)(po >> 8) != a;
          }
          return __ballot(bv);
        };
        const int clast = max(1, min((kWireBuyLo + max(nm, hm) - 1) >> 6, 16));
        uint64_t bprev = pm(kFoBuyLane + j);
#pragma unroll 1
        for (int cc = 2; cc <= clast; cc++) {  // Buy-only chunks, not tracked
          const uint64_t bcur = 64 * (cc - 1) < nm ? buy_word(cc - 1) : 0ull;
          fo_st(row, 64 * cc + lane, fo_bit(bcur << (kWireBuyLo & 63) | bprev >> (64 - (kWireBuyLo & 63))));
          bprev = bcur;
        }
        FO_STAMP(4);
#pragma unroll 1
        for (uint32_t cs = (chg >> 2) & 0x7Fu; cs; cs &= cs - 1u) {  // chunks 17 .. 23
          const int s = __builtin_ctz(cs);
          fo_st(row, 64 * (kFoTail0 + s) + lane, fo_bit(pm(10 * j + 2 + s)));
          nst += 64;
        }
        constexpr int kc = kFoChunks - 1, n = kMaskN - 64 * kc;  // + AgentId, CurrentTick (fo_put)
        if (chg >> 9) {
          const uint64_t m = pm(10 * j + 9);
          if (lane < n + 2) fo_st(row, 64 * kc + lane, lane < n ? fo_bit(m) : lane == n ? (float)aid : tickf);
          nst += n + 2;
        } else {
          if (lane == n + 1) fo_st(row, 64 * kc + lane, tickf);
          nst += 1;
        }
        nbytes += 4ull * (nst + 64 * (clast - 1));
      }
    } else if (!(NMMO_FO_ABL & 1)) {
      AoAgent ag;
      ag.a = a;
      ag.ti = tia;
      ag.r = r;
      ag.c = c;
      ag.gold = gold;
      ag.aid = aid;
      ag.nv = nv;
      ag.ninv = ninv;
      ag.prev_price = kWrap ? __builtin_amdgcn_readlane(my_prev, j) : -1;
      ag.mv = mv;
      const AoSections x = ao_sections<kWrap>(p, Ta, Spa, visw, ag, it);
      FO_STAMP(2);
      fg.ext = ext;
      fo_put<0>(row, fg, fo_chunk<0>(x), 0.f, 0.f);
      // Buy.MarketItem entry k < listings: exchange on, price <= gold, not the agent's own. buy_word
      // m = the ballot over listings 64 m + lane; chunk c holds words c - 1 (from bit 40) and c - 2
      // (its top 40 bits). Chunks 2..16 hold Buy entries only: written up to the known-zero
      // threshold max(nm, hm) (their entries past nm are zero).
      auto buy_word = [&](int m) {
        const int k = 64 * m + lane;
        bool bv = false;
        if (exch && k < nm) {
          const uint32_t po = mpo[k];
          bv = (int)(po & 255u) <= gold && (int)(po >> 8) != a;
        }
        return __ballot(bv);
      };
      const int nbuy = max(nm, hm);
      const int clast = max(1, min((kWireBuyLo + nbuy - 1) >> 6, 16));
      uint64_t bprev = nm > 0 ? buy_word(0) : 0ull;  // chunk 1: Attack.Target's tail, Buy's first 24
      fo_put<1>(row, fg, fo_chunk<1>(x) | bprev << (kWireBuyLo & 63), 0.f, 0.f);
      FO_STAMP(3);
#pragma unroll 1
      for (int cc = 2; cc <= clast; cc++) {  // Buy-only chunks, not tracked
        const uint64_t bcur = 64 * (cc - 1) < nm ? buy_word(cc - 1) : 0ull;
        fo_st(row, 64 * cc + lane, fo_bit(bcur << (kWireBuyLo & 63) | bprev >> (64 - (kWireBuyLo & 63))));
        bprev = bcur;
      }
      // chunk 17: Buy entries 984..1023 (word 15, only when nm > 960: the loop then ran to 16)
      FO_STAMP(4);
      const uint64_t buy17 = nm > 15 * 64 ? bprev >> (64 - (kWireBuyLo & 63)) : 0ull;
      fo_tail_chunks<kFoTail0>(row, fg, x, buy17, (float)aid, tickf);
      nbytes += 4ull * (fg.nst + 64 * (clast - 1));
    }
    FO_STAMP(5);
    // Entity rows: two per pass (lanes 0-30 row k, lanes 32-62 row k + 1: 62 contiguous floats),
    // the rows past the visible ones not known zero as one zero run
    const int nv2 = (nv + 1) & ~1;
    if (!(NMMO_FO_ABL & 2)) {
      const uint32_t de = kFlatEntity + (lane - eh);
      // the row / column lanes take the packed word's fields (their columns of T hold the item words)
      const bool epos = (lane & 31) == F_ROW || (lane & 31) == F_COL;
      const uint32_t esh = (lane & 31) == F_COL ? 16u : 0u;
      // kMirror: the first kFoGather rows from the gathered tile (lane = field: 128 contiguous bytes
      // per pass); the rows past them from the mirror in HBM, in a loop of their own (as the
      // listings past the staged ones below: the common path issues no global load)
      const int16_t* gj = gat + (size_t)(w * kPerWave + j) * kFoGather * kMirrorCols;
      const int nst2 = kMirror ? min(nv2, kFoGather) : nv2;
#pragma unroll 1
      for (int k0 = 0; k0 < nst2; k0 += 2) {
        const int k = k0 + eh;
        if (ef < NMMO_N_ENTITY_COLS) {
          float v = 0.f;
          if (k < nv) {
            const uint32_t vw = visw[k];
            const int tv = kMirror ? gj[k * kMirrorCols + ef] : T[ef * Sp + ao_slot(vw)];
            v = (float)(epos ? (int)((vw >> esh) & 255u) : tv);
          }
          fo_st(row, de + k0 * NMMO_N_ENTITY_COLS, v);
        }
      }
      if constexpr (kMirror) {
        if (nv2 > kFoGather) {
          const int16_t* Mk = kp->frows + (size_t)e * kMaxSlots * kMirrorCols;
#pragma unroll 1
          for (int k0 = kFoGather; k0 < nv2; k0 += 2) {
            const int k = k0 + eh;
            if (ef < NMMO_N_ENTITY_COLS) {
              float v = 0.f;
              if (k < nv) {
                const uint32_t vw = visw[k];
                const int tv = Mk[(size_t)min(ao_slot(vw), kMaxSlots - 1) * kMirrorCols + ef];
                v = (float)(epos ? (int)((vw >> esh) & 255u) : tv);
              }
              fo_st(row, de + k0 * NMMO_N_ENTITY_COLS, v);
            }
          }
        }
      }
      const int hz = max(nv2, hv);
      wave_zero(row, kFlatEntity + nv2 * NMMO_N_ENTITY_COLS, kFlatEntity + hz * NMMO_N_ENTITY_COLS);
      nbytes += 4ull * (hz * NMMO_N_ENTITY_COLS + max(nm, hm) * 16);
    }
    FO_STAMP(6);
    // Inventory: item q = 4 h + lane / 16, column lane % 16 (own items, owner = self); not stored
    // when the row was last written from the same 12 item words (its only inputs besides AgentId)
    bool inv_same;
    if constexpr (kMirror) {  // (compared by the mask pass)
      inv_same = ((uint32_t)(mp.idiff >> (kInv * j)) & ((1u << kInv) - 1u)) == 0u;
    } else {
      const int jl = (12 * j + lane) & 63;
      const uint32_t px = (uint32_t)__shfl((int)pinv.x, jl), py = (uint32_t)__shfl((int)pinv.y, jl);
      inv_same = ext && __ballot(lane < kInv && (px != it.x || py != it.y)) == 0ull;
    }
    if (!inv_same) {
      if constexpr (kMirror) ninv = __builtin_ctzll(~__ballot(lane < kInv && it_type(ist[la * kInv + min(lane, kInv - 1)]) != 0));
#pragma unroll
      for (int h = 0; h < ((NMMO_FO_ABL & 4) ? 0 : kInv * 16 / 64); h++) {
        const int q = 4 * h + iq;
        float v = 0.f;
        if (4 * h < ninv && q < ninv) v = ic_value(ist[la * kInv + q], aid, icd);  // (a uniform skip first)
        fo_st(row, kFlatInv + 64 * h + lane, v);
      }
      nbytes += 4ull * kInv * 16;
    }
    FO_STAMP(7);
    // Market (the env's listings, ascending row; owner = lister) and its zero run down to hm
    // (the listings past the staged ones in a loop of their own: a global load in the common loop
    // made every iteration wait for all of the row's stores -- vmcnt counts stores and retires in
    // order -- whether or not it took the load)
    const int nms = (NMMO_FO_ABL & 8) ? 0 : fo_staged(nm);
    for (int k = lane; k < nms * 16; k += 64) fo_st(row, kFlatMarket + k, ic_value(mtop[-(k >> 4)], (mpo[k >> 4] >> 8) + 1, icd));
    if (nm > nms && !(NMMO_FO_ABL & 8)) {
      for (int k = nms * 16 + lane; k < nm * 16; k += 64) {
        const int q = k >> 4;
        const int v = kp->mlist[(size_t)e * NMMO_MARKET_ROWS + q];
        const uint2 wd = kp->items[((size_t)e * P + ((v >> 16) & 255)) * kInv + ((v >> 24) & 15)];
        fo_st(row, kFlatMarket + k, ic_value(wd, (mpo[q] >> 8) + 1, icd));
      }
    }
    wave_zero(row, kFlatMarket + nm * 16, kFlatMarket + max(nm, hm) * 16);
    FO_STAMP(8);
    // Task: only when the row does not hold this task's embedding yet (read in place)
    const int task = __builtin_amdgcn_readlane(my_task, j);
    if (!((ztask >> j) & 1)) {
      // kFoTaskBatch loads in flight before their stores: each load waits for every store issued
      // before it (vmcnt retires in order), so a load-store loop drained the queue per 64 floats
      const float* temb = kp->task + (size_t)task * tdim;
      int k0 = 0;
      for (; k0 + kFoTaskBatch * 64 <= tdim; k0 += kFoTaskBatch * 64) {
        float t[kFoTaskBatch];
#pragma unroll
        for (int i = 0; i < kFoTaskBatch; i++) t[i] = temb[k0 + 64 * i + lane];
#pragma unroll
        for (int i = 0; i < kFoTaskBatch; i++) fo_st(row, kFlatTask + k0 + 64 * i + lane, t[i]);
      }
      for (int k = k0 + lane; k < tdim; k += 64) fo_st(row, kFlatTask + k, temb[k]);
      nbytes += 4ull * tdim;
    }
    FO_STAMP(9);
    // Tile: (row, column, material) per window tile t = lane + 64 i, three stores 12 B apart, all
    // three every step: the three stores of a pass fill 768 contiguous bytes, so the section goes out
    // as whole lines. (Round 5 skipped the row / column components when the agent had not moved: a
    // third of the stores, but every line of the section was still written in part, which HBM writes
    // as whole sectors -- WRITE_SIZE 1.9x the stored bytes; NMMO_FO_TILE_SKIP=1 keeps that variant.)
    const uint32_t ppos = (uint32_t)__builtin_amdgcn_readlane((int)(kMirror ? mp.lo : img.x), 40 + j);
    const bool tkn = NMMO_FO_TILE_SKIP && ext && !((ztile >> j) & 1);  // the Tile section holds what this kernel wrote
    const bool same_r = tkn && (int)(ppos & 255u) == r, same_c = tkn && (int)((ppos >> 8) & 255u) == c;
    if (!(NMMO_FO_ABL & 16)) {
      float* dt = row + kFlatTask + tdim + 3 * lane;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (lane + 64 * i < 225) {
          const float vr = (float)(r + ((toff[i] << 24) >> 24)), vc = (float)(c + (toff[i] >> 8)), vm = (float)wm[i];
          if (NMMO_FO_TILE_SKIP) {
            if (!same_r) dt[192 * i] = vr;
            if (!same_c) dt[192 * i + 1] = vc;
            dt[192 * i + 2] = vm;
          } else {  // the tile's 12 bytes as one 3-dword store (rows are 4-B aligned)
            typedef float f3 __attribute__((ext_vector_type(3)));
            const f3 v = {vr, vc, vm};
            __builtin_memcpy(dt + 192 * i, &v, 12);
          }
        }
      }
      nbytes += 4ull * 225 * (1 + !same_r + !same_c);
    }
    FO_STAMP(10);
    if constexpr (!kMirror) {  // the row's state: tag, zero thresholds and task, then the extended state
                               // (kMirror: written by the mask pass for the wave's agents at once)
      uint32_t* zx = reinterpret_cast<uint32_t*>(kp->zext + ((size_t)e * P + a) * kZext);
      int wv = fg.nimg;  // lanes 0..19 the tracked masks, lanes 20 / 21 the position
      if (lane == 20) wv = r | c << 8;
      if (lane == 21) wv = 0;
      if (lane < 22) zx[lane] = (uint32_t)wv;
      if (!inv_same && lane < kInv) reinterpret_cast<uint2*>(zx + 22)[lane] = it;
      if (lane == 0) {
        if (!zv) kp->zrow[(size_t)e * P + a] = kp->ztag;
        kp->zst[(size_t)e * P + a] = zs_pack(nv2, nm, task) | kZsExt;
      }
    }
#if NMMO_FO_STAMPS
    FO_STAMP(11);
    if (lane == 0 && (size_t)e * P + a < (1u << 17))
      for (int k = 0; k < kFoStamps; k++) fo_stamp_buf[(size_t)e * P + a][k] = fst[k];
#endif
    if constexpr (!kMirror) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the next agent reuses visw
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
#if NMMO_FO_STAMPS
  wst_[4] = __builtin_amdgcn_s_memtime();
  wst_[5] = (uint64_t)e | (uint64_t)nrows << 32;
  {
    const size_t wi = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kAoWaves + w;
    if (lane == 0 && wi < (1u << 15))
      for (int k = 0; k < 6; k++) fo_wave_buf[wi][k] = wst_[k];
  }
#endif
  if (p.rows_out && lane == 0 && nrows) {  // per env: one address per env keeps the atomics uncontended
    atomicAdd(&p.rows_out[2 * e], (unsigned long long)nrows);
    atomicAdd(&p.rows_out[2 * e + 1], nbytes);
  }
}

hipError_t launch_flat_obs(const ObsParams& p, hipStream_t stream) {
  if (!(p.obs && p.ztag && p.zrow)) return hipErrorInvalidValue;  // a tracked buffer only
  const int ne = list_grid(p.env_list, p.n_list, p.n_envs);
  if (ne <= 0) return hipSuccess;
#if NMMO_FO_XCD
  const dim3 grid(ne * ((p.P + kAoAgents - 1) / kAoAgents)), block(64 * kAoWaves);
#else
  const dim3 grid(ne, (p.P + kAoAgents - 1) / kAoAgents), block(64 * kAoWaves);
#endif
  const size_t lds = fo_lds_bytes(p.S);
  if (p.frows) {  // the tick's entity mirror of this state (step_impl: 384 slots only)
    if (!p.fpk || !p.zext || p.S != kMaxSlots) return hipErrorInvalidValue;
    if (p.wflags) hipLaunchKernelGGL((flat_obs_kernel<true, kMaxSlots, true, true>), grid, block, kFoMirrorLds, stream, p);
    else hipLaunchKernelGGL((flat_obs_kernel<false, kMaxSlots, true, true>), grid, block, kFoMirrorLds, stream, p);
  } else if (p.S == kMaxSlots) {
    if (p.wflags) hipLaunchKernelGGL((flat_obs_kernel<true, kMaxSlots>), grid, block, lds, stream, p);
    else hipLaunchKernelGGL((flat_obs_kernel<false, kMaxSlots>), grid, block, lds, stream, p);
  } else if (p.S % 8 != 0) {
    if (p.wflags) hipLaunchKernelGGL((flat_obs_kernel<true, 0, false>), grid, block, lds, stream, p);
    else hipLaunchKernelGGL((flat_obs_kernel<false, 0, false>), grid, block, lds, stream, p);
  } else {
    if (p.wflags) hipLaunchKernelGGL((flat_obs_kernel<true, 0>), grid, block, lds, stream, p);
    else hipLaunchKernelGGL((flat_obs_kernel<false, 0>), grid, block, lds, stream, p);
  }
  return hipGetLastError();
}

}  // namespace nmmo

#if NMMO_FO_STAMPS
// diagnostic export of the stamp variant only: copy the stamps out, then zero them
extern "C" __attribute__((visibility("default"))) int nmmo_debug_fo_stamps(void* host, size_t bytes) {
  if (bytes > sizeof(nmmo::fo_stamp_buf)) bytes = sizeof(nmmo::fo_stamp_buf);
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(nmmo::fo_stamp_buf), bytes) != hipSuccess) return -1;
  void* d = nullptr;
  if (hipGetSymbolAddress(&d, HIP_SYMBOL(nmmo::fo_stamp_buf)) != hipSuccess) return -1;
  return hipMemset(d, 0, sizeof(nmmo::fo_stamp_buf)) == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}
extern "C" __attribute__((visibility("default"))) int nmmo_debug_fo_wave_stamps(void* host, size_t bytes) {
  if (bytes > sizeof(nmmo::fo_wave_buf)) bytes = sizeof(nmmo::fo_wave_buf);
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(nmmo::fo_wave_buf), bytes) != hipSuccess) return -1;
  void* d = nullptr;
  if (hipGetSymbolAddress(&d, HIP_SYMBOL(nmmo::fo_wave_buf)) != hipSuccess) return -1;
  return hipMemset(d, 0, sizeof(nmmo::fo_wave_buf)) == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}
#endif
