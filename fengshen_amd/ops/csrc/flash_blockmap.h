// XCD-aware block map of the flash v3 kernels.
//
// The chip deals the blocks of a launch round-robin over its 8 XCDs by
// linear block id L = x + nx * (y + ny * z): blocks L and L + 8 share an
// XCD (observed behaviour, not a contract: a different placement costs
// speed, never correctness).  With the plain (x, head, batch) grid and
// nx == 8 (s = 2048) every block of one x therefore sits on one XCD, and
// under the causal mask a block's work grows with x (fwd, dq) or falls with
// it (dkv): one XCD gets 8/36 of the work, another 1/36.
//
// The map lists the logical blocks in the order (z, y) major, x minor, the
// heaviest x of a (z, y) column first, and gives the blocks of one label
// L % 8 a contiguous chunk of that list, in the order the chip starts them.
// Each XCD then runs whole (batch, head) columns: the work of two labels
// differs by at most one column, and a head's K/V (fwd, dq) or Q/dO (dkv)
// is fetched into one L2 instead of eight.  The chunks have q + 1 blocks
// for the first T % 8 labels and q = T / 8 for the rest, which is exactly
// how many ids with that label the chip deals, so the map is a bijection
// for every T, below 8 included.
#pragma once

// bindings.cpp fills its table with this function through the host compiler
#if defined(__HIPCC__)
#define FLASH_HD __host__ __device__
#else
#define FLASH_HD
#endif

#define FLASH_NXCD 8

struct FlashBlock {
  unsigned int x, y, z;
};

// Logical block of hardware linear block id L in the logical grid
// (nx, ny, nz).  heavy_last: the work of a block grows with x (else it
// falls), so the column is walked from nx - 1 down.
FLASH_HD inline FlashBlock flash_v3_block_of(unsigned int L, unsigned int nx,
                                             unsigned int ny, unsigned int nz,
                                             bool heavy_last) {
  const unsigned int T = nx * ny * nz;
  const unsigned int q = T / FLASH_NXCD, r = T % FLASH_NXCD;
  const unsigned int label = L % FLASH_NXCD, slot = L / FLASH_NXCD;
  const unsigned int first =
      label < r ? label * (q + 1) : r * (q + 1) + (label - r) * q;
  const unsigned int p = first + slot;   // position in the logical order
  const unsigned int col = p / nx, i = p % nx;
  FlashBlock blk;
  blk.x = heavy_last ? nx - 1 - i : i;
  blk.y = col % ny;
  blk.z = col / ny;
  return blk;
}
