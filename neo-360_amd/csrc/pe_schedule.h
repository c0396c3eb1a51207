// Who writes which position of the 96-wide positional encoding outside the unit sphere (mlp_tp_hpp.hip, PE_C == 4).
// Plain integer arithmetic, usable from host code (tests/test_pe_schedule_cpu.py builds it into a stand-alone program) and from
// the kernel.
//
// Positions (the pair order launch_tp_pack_hp packs): pair p = octave * 4 + coordinate (x, y, z, 1/r) holds sin at 2 p and cos at
// 2 p + 1, so octave o is the 8-half chunk o and coordinate c its elements 2 c, 2 c + 1; positions 80..83 are the identity
// features x, y, z, 1/r; 84..95 are zero padding.  Chunks 0..7 live in the first encoding tile, 8..11 in the second.
//
// 1/r does not depend on the source view.  ONCE PER TILE the four waves write its 10 pairs (wave q: octaves q, 4 + q, 8 + q),
// identity position 83 and the padding; ONCE PER VIEW they write the 30 pairs of x, y, z, split 8 / 8 / 7 / 7, and identity
// positions 80..82.  Every position has exactly one writer.
// The per-view slots are laid out so that everything but the octave is known per SLOT, at compile time: slots 0..5 of wave q are
// x, y, z of octave 2 q and of octave 2 q + 1 (the 24 pairs of the first tile; coordinate = slot % 3, three pairs = 12 contiguous
// bytes of a chunk), slots 6 and 7 hand out the six pairs of octaves 8 and 9 (second tile) one per wave: slot 6 to all four
// waves, slot 7 to waves 0 and 1.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEO_PS_HD __host__ __device__ __forceinline__
#else
#define NEO_PS_HD inline
#endif

namespace neo {
namespace pe_sched {

constexpr int WAVES = 4, OCTAVES = 10, COORDS = 4, WIDTH = 96;
constexpr int IDENT_POS = 2 * OCTAVES * COORDS;      // 80: x, y, z, 1/r
constexpr int PAD_POS = IDENT_POS + COORDS;          // 84..95: zeros
constexpr int VIEW_PAIRS = OCTAVES * (COORDS - 1);   // 30 view-dependent pairs
constexpr int VIEW_SLOTS = (VIEW_PAIRS + WAVES - 1) / WAVES;     // 8: slots of the busiest wave
constexpr int VIEW_LOW_SLOTS = 2 * (COORDS - 1);                 // 6: slots 0..5 = two whole octaves below 8 per wave
constexpr int TILE_SLOTS = (OCTAVES + WAVES - 1) / WAVES;        // 3
constexpr int VIEW_IDENT_WAVE = 3;                   // a 7-pair wave writes x, y, z (positions 80..82) every view
constexpr int TILE_IDENT_WAVE = 2;                   // a 2-pair wave writes 1/r (position 83) and 84..87 once per tile,
constexpr int TILE_PAD_WAVE = 3;                     // the other one 88..95

// first position (the sine's; the cosine follows) of the pair of octave `oct`, coordinate `coord`
NEO_PS_HD constexpr int pair_pos(int oct, int coord) { return 2 * (oct * COORDS + coord); }

// ---- per view: x, y, z ----
NEO_PS_HD constexpr int view_pairs(int wave) { return VIEW_LOW_SLOTS + 1 + (wave < VIEW_PAIRS - WAVES * (VIEW_LOW_SLOTS + 1) ? 1 : 0); }
// index 0..5 into the pairs of octaves 8 and 9 (octave-major) for slots 6 and 7
NEO_PS_HD constexpr int view_high(int wave, int slot) { return (slot - VIEW_LOW_SLOTS) * WAVES + wave; }
// valid for slot < view_pairs(wave)
NEO_PS_HD constexpr int view_octave(int wave, int slot) {
    return slot < VIEW_LOW_SLOTS ? 2 * wave + slot / (COORDS - 1) : 2 * WAVES + view_high(wave, slot) / (COORDS - 1);
}
NEO_PS_HD constexpr int view_coord(int wave, int slot) {
    return slot < VIEW_LOW_SLOTS ? slot % (COORDS - 1) : view_high(wave, slot) % (COORDS - 1);
}

// ---- per tile: 1/r ----
NEO_PS_HD constexpr int tile_pairs(int wave) { return OCTAVES / WAVES + (wave < OCTAVES % WAVES ? 1 : 0); }
NEO_PS_HD constexpr int tile_octave(int wave, int slot) { return wave + WAVES * slot; }      // valid for slot < tile_pairs(wave)

}  // namespace pe_sched
}  // namespace neo
