"""The grid and the LDS tile of the level histogram's fold kernel (scanner_amd/csrc/scn_levels.hip), restated as tests/trace_caps.py
restates the trace's: a stated number of workgroups per CU -- not an occupancy query --, so a test can size the batch that takes
every team through its loop twice (the case that finds a tile not zeroed between a team's units), and a stated tile, so a test can
choose grids whose units fit it and grids whose units do not.  tests/test_levels_cpu.py holds each number to the launcher's line.

  kernel                     launcher (file)                            workgroups
  scn_levels_fold_kernel     scn_launch_levels_fold (scn_levels.hip)    min(ceil(units / teams), CUs * per_cu): a team per unit and trip;
                                                                        n <= 512: 4 teams (waves) per 256-thread workgroup, 8 per CU;
                                                                        n <= 4096: one team of 256, 8 per CU; above: one of 1024, 2 per CU
"""
LEVELS_BLOCKS_PER_CU = {256: 8, 1024: 2}   # `constexpr int kLevelsBlocksPerCu256 = 8, kLevelsBlocksPerCu1024 = 2;`
LEVELS_TILE_WORDS = {256: 4096, 1024: 8192}  # `constexpr int kLevelsTileWords256 = 4096, kLevelsTileWords1024 = 8192;`
LDS_BYTES_PER_CU = 160 * 1024
KEYS = 256  # `constexpr uint32_t kLevelsKeys = 256u;` (scn_levels.h)


def levels_team(n):
    """threads of the team that works one unit of n points: `if (a.n <= 512u)` 64, `if (a.n <= 4096u)` 256, else 1024"""
    return 64 if n <= 512 else 256 if n <= 4096 else 1024


def _block(n):
    team = levels_team(n)
    return 256 if team == 64 else team  # scn_detect.h, Team<T>::BLOCK


def levels_cap(num_cus, n):
    """units one trip of the fold kernel's loop takes: a team each, over the whole grid"""
    return num_cus * LEVELS_BLOCKS_PER_CU[_block(n)] * (_block(n) // levels_team(n))


def tile_cells(n, n_edges):
    """consecutive cells a team's tile covers: `TILE = BLOCK_TILE / G::TEAMS`, `tile_cells = TILE / n_levels`"""
    return LEVELS_TILE_WORDS[_block(n)] // (_block(n) // levels_team(n)) // (n_edges + 1)
