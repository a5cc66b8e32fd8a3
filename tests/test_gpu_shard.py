"""Multi-GPU path (config 5), functional checks on ONE GPU: 2, 4 and 8 ranks share cuda:0 and solve a lattice by
nested-dissection subtree sharding through aprilsam_amd_shard_* (exchange inside the library; host-callback transport
over gloo here because RCCL cannot place two ranks on one device).  Checked: chi^2 per iteration against the reference
golden (K = 24, 316) or the recorded single-GPU trace (K = 1000), the gathered STATES against a single-GPU run of the
same iterations (<= 1e-9), identical gathered states on every rank, and that a rank only
allocates the fronts it owns.  On the 8-GPU node the same calls run with the RCCL transport (world = 1 exercises it
here).  These are the only tests on the gloo and RCCL wires; what the lattices never reach (idle ranks, primary-child ghosts,
several roots, 3 and 5 ranks, the failure contracts, ...) is in tests/test_gpu_shard_designs.py, with the ranks as threads of
one process."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, K, iters, out, backend="gloo", env=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.update(env or {})
    sys.path.insert(0, ROOT)
    import zlib
    import torch.distributed as dist
    from aprilsam_amd import host
    from aprilsam_amd.shard import ShardedSolver
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lib = host.SolverLib()
    if (env or {}).get("ONE_DEVICE_PER_RANK"):
        assert lib.dll.aprilsam_amd_set_device(rank) == 0        # (before the first solver call: this rank's contexts live on device `rank`)
    g = lib.new_graph(); lib.dll.aprilsam_amd_make_lattice(g.ptr, K); p = lib.new_param()
    pretend = (env or {}).get("PRETEND_RCCL_UNAVAILABLE_ON")
    sol = ShardedSolver(lib, g, p, rank, world, backend=backend, _pretend_rccl_unavailable_on=pretend)
    if pretend is not None:
        assert sol.transport_note and "host callbacks over gloo" in sol.comm_info()["transport"], sol.comm_info()
    if (env or {}).get("ONE_DEVICE_PER_RANK"):
        ci = sol.comm_info()                                     # the wire really is RCCL, one rank per device
        assert ci["transport"].startswith("RCCL") and ci["ncclCommCount"] == world and ci["ncclCommUserRank"] == rank and ci["hip_device"] == rank, ci
    chi2 = [sol.chi2()]
    for _ in range(iters):
        sol.iterate(1)
        chi2.append(sol.chi2())
    st = sol.gather_states()
    owned_fronts = int((sol.owner == rank).sum())
    digest = zlib.crc32(np.ascontiguousarray(st).tobytes())
    if rank == 0:
        np.save(os.path.join(ROOT, "gpurun_out", f"shard_states_{K}_{world}.npy"), st)
    out.put((rank, chi2, owned_fronts, int(sol.n_fronts), len(sol.xfer), sol.comm_bytes_per_iteration(), digest,
             sol.pool_doubles, sol.pool_doubles_all))
    sol.close(); p.destroy(); g.destroy()
    dist.barrier(); dist.destroy_process_group()


def _run(world, K, iters, timeout=900, backend="gloo", env=None):
    import torch.multiprocessing as mp
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = 29600 + os.getpid() % 2000 + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, K, iters, out, backend, env)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted(out.get(timeout=timeout) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    st = np.load(os.path.join(ROOT, "gpurun_out", f"shard_states_{K}_{world}.npy"))
    return res, st


def _single_gpu_states(lib, K, iters):
    g = lib.new_graph(); lib.dll.aprilsam_amd_make_lattice(g.ptr, K); p = lib.new_param()
    chi2, _ = g.batch_resident(p, iters)
    st = g.states()
    p.destroy(); g.destroy()
    return chi2, st


def _check(res, st, world, chi2_want, st_want):
    nf = res[0][3]
    for rank, chi2, owned, nfr, nx, comm, digest, pool, pool_all in res:
        assert np.max(np.abs(np.array(chi2) - chi2_want) / chi2_want) < 1e-9, (rank, chi2, chi2_want)
        assert 0 < owned < nf and nx >= world - 1
        assert digest == res[0][6]                            # every rank gathered bit-identical states
        assert pool < 0.8 * pool_all                          # a rank allocates what it owns (+ ghosts), not the whole plan
    assert sum(r[2] for r in res) == nf                       # every front has exactly one owner
    assert sum(r[7] for r in res) < 1.35 * res[0][8]          # ... and the ghosts add little
    assert np.max(np.abs(st - st_want)) < 1e-9


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_small_lattice_matches_reference_golden(built, lib, world):
    K = 24
    G = np.load(os.path.join(ROOT, "tests", "golden", f"lattice_{K}.npz"))
    iters = len(G["chi2"]) - 1
    res, st = _run(world, K, iters)
    c1, s1 = _single_gpu_states(lib, K, iters)
    assert np.max(np.abs(c1 - G["chi2"]) / G["chi2"]) < 1e-6
    _check(res, st, world, G["chi2"], s1)
    assert np.max(np.abs(st - G["final_states"])) < 1e-6


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_100k_lattice_matches_reference_golden_and_single_gpu_states(built, lib, world):
    """config 4's graph (99 856 poses) across 2 / 4 / 8 ranks: chi^2 against the reference's own numbers, states against
    the single-GPU run"""
    K = 316
    G = np.load(os.path.join(ROOT, "tests", "golden", "lattice_316.npz"))
    iters = len(G["chi2"]) - 1
    res, st = _run(world, K, iters)
    c1, s1 = _single_gpu_states(lib, K, iters)
    assert np.max(np.abs(c1 - G["chi2"]) / G["chi2"]) < 1e-9
    _check(res, st, world, G["chi2"], s1)
    assert np.max(np.abs(st[::997] - G["states_sample"])) < 1e-6      # the reference's own states after that iteration


@pytest.mark.parametrize("world", [2, 8])
def test_sharded_1m_lattice_matches_the_single_gpu_trace(built, lib, world):
    """config 5 (10^6 poses / 3 994 003 factors) across 2 and 8 ranks on one GPU: chi^2 after 0, 1, 2 iterations against
    bench.LATTICE1M_CHI2's single-GPU values, gathered states against a single-GPU run"""
    import bench
    res, st = _run(world, 1000, 1, timeout=1500)
    c1, s1 = _single_gpu_states(lib, 1000, 1)
    want = np.array(bench.LATTICE1M_CHI2[:2])
    assert np.max(np.abs(c1 - want) / want) < 1e-9
    _check(res, st, world, want, s1)
    _normal_equations_hold(lib, 1000, st)


def _normal_equations_hold(lib, K, st_after_one_iteration):
    """... and against nothing but the inputs: dx = gathered states - initial states (theta wrapped) solves the reference's normal equations
    at the initial states (tests/support/normal_eq.py; the subtraction costs eps x |coordinate| ~ 1e-13 of dx)"""
    from tests.support.normal_eq import normal_equation_residual
    arr = lib.lattice_arrays(K)
    dx = st_after_one_iteration - arr[0]
    dx[:, 2] = (dx[:, 2] + np.pi) % (2 * np.pi) - np.pi
    out = normal_equation_residual(arr[0], arr[1], arr[2], arr[3], arr[4], dx, 1e-4)
    assert out["rel_max"] < 1e-9, out


def test_rccl_unavailable_on_one_rank_falls_back_to_host_callbacks_everywhere(built, lib):
    """the launcher asks for the RCCL transport, rank 1 cannot load RCCL: every rank must notice BEFORE the collective
    communicator set-up (a rank missing from ncclCommInitRank would hang the others) and the run continues over the
    host-callback transport on a gloo group, with the same results"""
    K = 24
    G = np.load(os.path.join(ROOT, "tests", "golden", f"lattice_{K}.npz"))
    iters = len(G["chi2"]) - 1
    res, st = _run(2, K, iters, backend="nccl", env={"PRETEND_RCCL_UNAVAILABLE_ON": "1"})
    c1, s1 = _single_gpu_states(lib, K, iters)
    _check(res, st, 2, G["chi2"], s1)


@pytest.mark.parametrize("K", [316, 1000])
def test_rccl_wire_between_devices(built, lib, K):
    """Config 5 as BASELINE.json states it -- one rank per MI355X, Schur slabs and separator solutions over RCCL / xGMI --
    on as many devices as the box has (2, 4 or 8): auto-skips on a single-GPU box (the builder's and the round-end test
    machine), so that the first multi-GPU box that runs this suite exercises the wire: RCCL reports one rank per device,
    chi^2 equals the single-GPU trace to 1e-9 and the gathered states a single-GPU run to 1e-9, bit-identical on every rank."""
    ndev = lib.device_count()
    if ndev < 2:
        pytest.skip(f"{ndev} HIP device(s) visible: the RCCL wire needs at least two")
    world = 8 if ndev >= 8 else 4 if ndev >= 4 else 2
    if K == 316:
        G = np.load(os.path.join(ROOT, "tests", "golden", "lattice_316.npz"))
        want = G["chi2"]; iters = len(want) - 1
    else:
        import bench
        want = np.array(bench.LATTICE1M_CHI2[:2]); iters = 1
    res, st = _run(world, K, iters, timeout=1500, backend="nccl", env={"ONE_DEVICE_PER_RANK": "1"})
    c1, s1 = _single_gpu_states(lib, K, iters)
    _check(res, st, world, want, s1)


def test_rccl_transport_on_one_rank(built, lib):
    """world = 1 over the RCCL transport: librccl.so loads, the communicator initialises on the library's device, the
    gather's all-reduce and the chi^2 sum run through RCCL on the solver stream; results equal the resident path"""
    from aprilsam_amd.shard import ShardedSolver
    K = 60
    G = np.load(os.path.join(ROOT, "tests", "golden", f"lattice_{K}.npz"))
    g = lib.new_graph(); lib.dll.aprilsam_amd_make_lattice(g.ptr, K); p = lib.new_param()
    sol = ShardedSolver(lib, g, p, 0, 1, backend="nccl")
    chi2 = [sol.chi2()]
    for _ in range(len(G["chi2"]) - 1):
        sol.iterate(1); chi2.append(sol.chi2())
    st = sol.gather_states()
    assert np.max(np.abs(np.array(chi2) - G["chi2"]) / G["chi2"]) < 1e-9
    assert np.max(np.abs(st - G["final_states"])) < 1e-6
    assert abs(sol.pool_doubles - sol.pool_doubles_all) <= 32 * sol.n_fronts      # (alignment padding only)
    sol.close(); p.destroy(); g.destroy()
