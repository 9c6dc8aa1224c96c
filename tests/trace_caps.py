"""The grid of the sweep trace's fold kernel (scanner_amd/csrc/scn_trace.hip), restated as tests/launch_caps.py restates the other
persistent launchers': a stated number of workgroups per CU -- not an occupancy query --, so a test can size the batch that takes
every team through its loop twice.  tests/test_trace_cpu.py holds each number to the launcher's line.

  kernel                     launcher (file)                           workgroups
  scn_trace_fold_kernel      scn_launch_trace_fold (scn_trace.hip)     min(ceil(units / teams), CUs * per_cu): a team per unit and trip;
                                                                       n <= 512: 4 teams (waves) per 256-thread workgroup, 8 per CU;
                                                                       n <= 4096: one team of 256, 8 per CU; above: one of 1024, 2 per CU
"""
TRACE_BLOCKS_PER_CU = {256: 8, 1024: 2}  # `constexpr int kTraceBlocksPerCu256 = 8, kTraceBlocksPerCu1024 = 2;`


def trace_team(n):
    """threads of the team that works one unit of n points: `if (a.n <= 512u)` 64, `if (a.n <= 4096u)` 256, else 1024"""
    return 64 if n <= 512 else 256 if n <= 4096 else 1024


def trace_cap(num_cus, n):
    """units one trip of the fold kernel's loop takes: a team each, over the whole grid"""
    team = trace_team(n)
    block = 256 if team == 64 else team  # scn_detect.h, Team<T>::BLOCK
    return num_cus * TRACE_BLOCKS_PER_CU[block] * (block // team)
