// ABI version of libdca_hip.so: bumped whenever an entry point of include/dca_hip.h changes its argument list, so a
// stale binary (the .so is git-ignored and shipped separately) is refused by the ctypes loader instead of being called
// with the wrong arguments.
#include "dca_common.h"

extern "C" int dca_abi_version(void) { return DCA_ABI_VERSION; }

// the persistent tile walk (dca_tiles.h) of workgroup wg, for host callers: walk = {begin, end, step}
extern "C" int dca_tile_walk(long tiles, int grid, int wg, int* walk) {
  DCA_REQUIRE(walk && tiles >= 0 && tiles < DCA_TILES_END && grid > 0 && wg >= 0 && wg < grid);
  const DcaTileWalk w = dca_tile_walk_of(tiles, (unsigned)grid, (unsigned)wg);
  walk[0] = w.begin; walk[1] = w.end; walk[2] = w.step;
  return 0;
}
