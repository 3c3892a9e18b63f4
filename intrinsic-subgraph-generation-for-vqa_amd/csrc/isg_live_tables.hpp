// One masked tile's table set as gatv2_layer_conv_groups_kernel (csrc/isg_layer_conv.hip) keeps it in LDS, and as
// layer_conv_live_tables_kernel (csrc/isg_live_tables.hip) writes it to memory: the same bytes at the same offsets, so that the
// layer kernel's fetch is a copy.  Declared once, for both files.
#pragma once

namespace isg {

constexpr int LT_ROWS = 64, LT_ECAP = 256;             // a tile's node rows and CSR slots (LC_ROWS, LC_ECAP)
// offset 0:                                              [256] int2 {eid, mask bits}
constexpr int LG_T_LG = LT_ECAP * 8;                   // [256] float: +0 for a dead slot, the edge planes' inverse scale for a live one
constexpr int LG_T_SP = LG_T_LG + LT_ECAP * 4;         // [256] byte: source tile row
constexpr int LG_T_DR = LG_T_SP + LT_ECAP;             // [256] byte: destination tile row
constexpr int LG_T_LV = LG_T_DR + LT_ECAP;             // [256] byte: the tile's live slots in CSR order
constexpr int LG_T_RP = LG_T_LV + LT_ECAP;             // [68] int: row pointers relative to the tile's first slot
constexpr int LG_T_POS = LG_T_RP + 68 * 4;             // [64] byte: in LDS tile row -> list position (group-dependent); in memory the header
constexpr int LG_TILE_BYTES = LG_T_POS + 64;
// the header of an image in memory, in the bytes of the POS field
constexpr int LG_H_DESC = LG_T_POS;                    // int4 {r0, min(nrows, 64), e0, min(ne, 256)}
constexpr int LG_H_TOUCH = LG_T_POS + 16;              // uint64: tile rows that a live slot's source or destination names; then 8 zero bytes
constexpr int LG_H_LIVE = LG_T_POS + 32;               // uint64 [4]: live-slot bit words (bit s & 63 of word s >> 6)
static_assert(LG_TILE_BYTES % 16 == 0 && LG_T_RP % 16 == 0 && LG_T_POS % 16 == 0, "16-byte pieces");
static_assert(LG_TILE_BYTES == 4176 && LG_H_LIVE + 32 == LG_TILE_BYTES, "the image layout include/isg_masked.h documents");

}  // namespace isg
