// obs_layout.h — the one compile-time definition of the observation row layouts: the flat float32
// row (SPEC.md §8, pufferlib's sorted-key order) and the int16 part of the native row (SPEC §8b).
// Every kernel and nmmo_layout (capi.hip) derive their offsets from here; only the Task width
// (NmmoConfig::task_embed_dim) is a run-time value, and it moves only the Tile offset and the row
// length. Independent restatements: oracle/nmmo_cpu_abi.c and nmmo_amd/layout.py
// (tests/test_layout.py compares the three).
#pragma once

#include "common.h"

namespace nmmo {

constexpr int kItemCols = 16;                   // Inventory / Market columns
constexpr int kWinTiles = 225, kTileCols = 3;   // the 15 x 15 window: (row, col, material) per tile

// The 12 ActionTargets sections in flat order (Attack.Style, Attack.Target, Buy.MarketItem,
// Destroy, Give.InventoryItem, Give.Target, GiveGold.Price, GiveGold.Target, Move, Sell.InventoryItem,
// Sell.Price, Use) and their flat entry offsets; sec_wire: offsets with Buy.MarketItem left out.
constexpr int kSecN[kHeads] = {3, kNObs + 1, NMMO_MARKET_ROWS + 1, kInv + 1, kInv + 1, kNObs + 1,
                               99, kNObs + 1, 5, kInv + 1, 99, kInv + 1};
__host__ __device__ constexpr int sec_flat(int k) { return k == 0 ? 0 : sec_flat(k - 1) + kSecN[k - 1]; }
__host__ __device__ constexpr int sec_wire(int k) { return k < 2 ? sec_flat(k) : sec_flat(k) - kSecN[2]; }
constexpr int kMkStyle = sec_flat(0), kMkAttackT = sec_flat(1), kWireBuyLo = sec_flat(2), kWireBuyN = kSecN[2],
              kMkDestroy = sec_flat(3), kMkGiveI = sec_flat(4), kMkGiveT = sec_flat(5), kMkGoldP = sec_flat(6),
              kMkGoldT = sec_flat(7), kMkMove = sec_flat(8), kMkSellI = sec_flat(9), kMkSellP = sec_flat(10),
              kMkUse = sec_flat(11);
constexpr int kMaskN = sec_flat(kHeads);  // ActionTargets entries: 1,586

// flat row: ActionTargets | AgentId | CurrentTick | Entity | Inventory | Market | Task | Tile
constexpr int kFlatId = kMaskN, kFlatTick = kFlatId + 1, kFlatEntity = kFlatTick + 1,
              kFlatInv = kFlatEntity + kNObs * NMMO_N_ENTITY_COLS, kFlatMarket = kFlatInv + kInv * kItemCols,
              kFlatTask = kFlatMarket + NMMO_MARKET_ROWS * kItemCols;
constexpr int kTileN = kWinTiles * kTileCols;
__host__ __device__ constexpr int flat_tile(int task_dim) { return kFlatTask + task_dim; }
__host__ __device__ constexpr int flat_elems(int task_dim) { return flat_tile(task_dim) + kTileN; }

// native row: NMMO_NATIVE_MASK_BYTES of u8 ActionTargets (flat entry order), then NMMO_NATIVE_I16
// int16: AgentId, CurrentTick | Entity | Inventory | Tile | task index | zero pad; per env P rows,
// then the Market rows
constexpr int kNatEntity = 2, kNatInv = kNatEntity + kNObs * NMMO_N_ENTITY_COLS,
              kNatTile = kNatInv + kInv * kItemCols, kNatTask = kNatTile + kTileN;
static_assert(kMaskN <= NMMO_NATIVE_MASK_BYTES && kNatTask < NMMO_NATIVE_I16, "native row holds its parts");
static_assert(NMMO_NATIVE_MARKET_BYTES == NMMO_MARKET_ROWS * kItemCols * 2, "native Market rows");
__host__ __device__ constexpr size_t native_env_bytes(int P) {
  return (size_t)P * NMMO_NATIVE_ROW_BYTES + NMMO_NATIVE_MARKET_BYTES;
}

}  // namespace nmmo
