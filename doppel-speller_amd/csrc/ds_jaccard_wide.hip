// The Jaccard kernels in their WIDE geometry: 2 workgroups of 512 threads per CU, tiles of 28672 truth rows (56 KiB of
// packed scores per workgroup) -- truth sets above ds::kNarrowMaxTruth rows, where the number of tiles per query counts.
#include "doppel_amd.h"
#define DS_GEOMETRY_NAME wide
#define DS_TILE_ROWS ds::kWideTileRows
#define DS_THREADS 512
#define DS_WGS_PER_CU 2
#define DS_CANDIDATES 1472  // 512 bytes go to the raw entries' tile bytes (epochs of 4 tiles), 1.6 KiB to the item directory
#define DS_PTR_TILES 3
#define DS_EPOCH_TILES 16  // round 5 at the C5 shape (20k queries x 50M rows, top-100): 152.6 (4) / 145.8 (8) / 144.1 ms (16); round 3 (40k queries): 361.2 (4) / 349.2 (8) / 347.4 ms (16); round 2 at the C3 shape: 91.1 (1) / 88.9 (2) / 86.5 (4) / 85.9 ms (8)
#include "ds_jaccard_impl.inc"
