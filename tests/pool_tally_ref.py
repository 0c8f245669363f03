"""NumPy restatements of the pool book-keeping kernels (csrc/azul_policy.hpp: azul_league_tally_kernel, azul_arena_tally_kernel), shared by
the lockstep-emulation tests (tests/test_league_host.py, tests/test_arena_host.py) and the device test (tests/test_gpu_pool_tally.py).
Every addition is one fp64 addition in the kernels' stated order, so the results are compared byte for byte."""
import numpy as np

GROUP = 16


def league_tally_ref(ep, ss, mark_ep, mark_ss, member, K, results):
    """The kernel restated: per member, games in ascending order, one fp64 addition per game and column; then the marks move up."""
    results, mark_ep, mark_ss = results.copy(), mark_ep.copy(), mark_ss.copy()
    for m in range(K):
        for grp, mg in enumerate(member):
            if min(int(mg), K - 1) != m:
                continue
            for g in range(grp * GROUP, min(len(ep), (grp + 1) * GROUP)):
                results[m, 0] = results[m, 0] + np.float64(int(ep[g]) - int(mark_ep[g]))
                for j in range(10):
                    results[m, 1 + j] = results[m, 1 + j] + (ss[g, j] - mark_ss[g, j])
                mark_ep[g] = ep[g]
                mark_ss[g] = ss[g]
    return results, mark_ep, mark_ss


def arena_tally_ref(ep, ss, mark_ep, mark_ss, agent, opp, K, results):
    """The stated order: per cell [a][o] the games of its groups in ascending order, one fp64 addition per game and column."""
    results = results.copy()
    for grp in range(len(agent)):
        a, o = min(int(agent[grp]), K - 1), min(int(opp[grp]), K - 1)
        for g in range(grp * GROUP, min(len(ep), (grp + 1) * GROUP)):
            results[a, o, 0] = results[a, o, 0] + np.float64(int(ep[g]) - int(mark_ep[g]))
            for j in range(10):
                results[a, o, 1 + j] = results[a, o, 1 + j] + (ss[g, j] - mark_ss[g, j])
    return results
