"""The rate of the solution branches (ezpz_system_solve_branches_device, ezpz_branch_cluster_device), printed as the
text of profiles/branches_rate.txt: samples per second of the run against the same starts and solves done through the public chain
with the answers brought to the host, the share of a run that is not the solve, and what the election costs.

Per system (blocks(3) of tests/branch_ref.py, 18 variables; chain(38), a connected sketch of 80 variables, compared on its first three
apexes: 8 branches) and per number of samples of one base:
  run          ezpz_system_solve_branches_device in the library's rounds, info and the branch records read back
  solve alone  the rounds' ezpz_system_solve_batch_device calls on ready starts (the run's own first 65536, in every round): what the
               run adds -- starts, assign, elect -- is the rest
  host chain   ezpz_mc_sample -> System.solve_batch with the answers on the host: the chain's first two links.  Its third, the
               clustering on the host, is NOT in the time (tests/branch_ref.py is a Python loop; it is timed at 4096 samples only)
Then the clustering alone (ezpz_branch_cluster_device) on made-up answers of 18 variables in 2, 8 and 32 tight clusters:
  fresh round  1024 samples of one base: no leaders yet, so the election kernel does everything (two memsets and that kernel)
  one base     1048576 samples of one base: every round's election is one workgroup
  16 bases     65536 samples of each of 16 bases: the same samples, sixteen electing workgroups

Host clock around work that ends in a synchronise; WARMUP untimed runs of each form, then REPEATS timed runs, the forms alternating;
median (min .. max).

    python tools/branches_rate.py > profiles/branches_rate.txt
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch  # (before the library: torch brings its own HIP runtime and must be the first to load one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import branch_ref as R  # noqa: E402
import ezpz_amd as E  # noqa: E402
from ezpz_amd._lib import BRANCH_DTYPE, BRANCH_INFO_DTYPE, STATUS_DTYPE  # noqa: E402

WARMUP, REPEATS, HOST_REPEATS = 1, 5, 2
SAMPLES = (4096, 1048576)
CHUNK, FIRST_ROUND = 65536, 1024  # the library's rounds (csrc/branches.hip)
SEED, MAX_BRANCHES = 11, 32


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def line(what, ts, samples, extra=""):
    ts = np.asarray(ts)
    print("   %-12s %10.3f ms (%.3f .. %.3f)  %12.0f samples/s%s" % (what, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3,
                                                                   samples / np.median(ts), extra))
    sys.stdout.flush()


def rounds(samples):
    first = 0
    while first < samples:
        count = min(FIRST_ROUND if first == 0 else CHUNK, samples - first)
        yield first, count
        first += count


def outputs(batch, n_vars):
    return [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (batch * BRANCH_INFO_DTYPE.itemsize, batch * MAX_BRANCHES * BRANCH_DTYPE.itemsize,
                                                                      batch * MAX_BRANCHES * n_vars * 8)]


def run_case(name, f, half_width, compare, samples, stream):
    system = E.System(f.records, f.n_vars)
    solved, st, _ = system.solve_batch(f.x0[None])
    assert st["converged"][0] == 1 and st["n_unsatisfied"][0] == 0, name
    x0_host, n = solved[0], f.n_vars
    dists = [E.McDist(*t) for t in f.spread(half_width)]
    L, cfg, h = E.lib(), C.byref(E.Config()._c()), stream.cuda_stream
    with torch.cuda.stream(stream):
        x0 = torch.from_numpy(x0_host).cuda()
        out = outputs(1, n)
        ready = E.mc_sample(SEED, dists, x0_host, 0, min(samples, CHUNK))  # (the run's own first starts, every round's stand-in)
        x_in = torch.from_numpy(ready).cuda()
        x_out = torch.zeros_like(x_in)
        status = torch.zeros((min(samples, CHUNK), STATUS_DTYPE.itemsize // 4), dtype=torch.int32, device="cuda")
    result = {}

    def run():
        with torch.cuda.stream(stream):
            system.solve_branches_device(x0.data_ptr(), dists, 1, samples, *(t.data_ptr() for t in out), seed=SEED, compare=compare,
                                         branch=E.BranchConfig(max_branches=MAX_BRANCHES), stream=h)
            result["info"] = out[0].cpu().numpy().view(BRANCH_INFO_DTYPE)
            result["branches"] = out[1].cpu().numpy().view(BRANCH_DTYPE)

    def solve_alone():
        for _, count in rounds(samples):
            rc = L.ezpz_system_solve_batch_device(system._h, x_in.data_ptr(), count, cfg, x_out.data_ptr(), status.data_ptr(), None, None, 0, h)
            assert rc == 0, rc

    def host_chain():
        starts = E.mc_sample(SEED, dists, x0_host, 0, samples)
        starts[0] = x0_host
        result["host"] = system.solve_batch(starts)[:2]

    forms = [run, solve_alone]
    for _ in range(WARMUP):
        for g in forms:
            timed(g)
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, g in enumerate(forms):
            ts[i].append(timed(g))
    timed(host_chain)
    th = [timed(host_chain) for _ in range(HOST_REPEATS)]
    info, me, ms = result["info"][0], np.median(ts[0]), np.median(ts[1])
    print("-- %s; %d samples of one base, uniform +-%g around its solved state, %d of %d variables compared"
          % (name, samples, half_width, n if compare is None else int(np.count_nonzero(compare)), n))
    print("   ok %d of %d; %d branches, overflow %d; counts %s" % (info["n_ok"], samples, info["n_branches"], info["n_overflow"],
                                                                 result["branches"]["count"][: int(info["n_branches"])].tolist()))
    line("run", ts[0], samples)
    line("solve alone", ts[1], samples, "   not the solve: %.1f%% of the run" % (100.0 * (1.0 - ms / me)))
    line("host chain", th, samples, "   run x%.2f, its clustering not included" % (np.median(th) / me))
    if samples <= 4096:
        x, st = result["host"]
        t0 = time.perf_counter()
        ref = R.cluster(x, R.ok_of(st["converged"], st["n_unsatisfied"]), compare=compare, max_branches=MAX_BRANCHES, origin=x0_host)
        print("   (the clustering of these %d answers by tests/branch_ref.py: %.1f ms, %d branches)"
              % (samples, (time.perf_counter() - t0) * 1e3, ref[0]["n_branches"][0]))


def cluster_case(n_clusters, stream):
    n, h, L = 18, stream.cuda_stream, E.lib()
    from ezpz_amd._lib import CBranchConfig

    bc = CBranchConfig(0, 0, MAX_BRANCHES, 1e-5, 1e-5)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n_clusters)
    shapes = [("fresh round", 1, 1024), ("one base", 1, 1048576), ("16 bases", 16, 65536)]
    data = {}
    with torch.cuda.stream(stream):
        for what, batch, samples in shapes:
            centre = torch.randint(0, n_clusters, (batch, samples, 1), device="cuda", generator=gen).double()
            x = (centre * 4.0 + torch.arange(n, device="cuda").double()).contiguous()  # tight clusters, 4 apart in every variable
            data[what] = (x, outputs(batch, n))

    def form(what, batch, samples):
        x, out = data[what]

        def call():
            rc = L.ezpz_branch_cluster_device(x.data_ptr(), None, None, batch, samples, n, C.byref(bc), *(t.data_ptr() for t in out), None, h)
            assert rc == 0, rc

        return call

    forms = [form(*s) for s in shapes]
    for _ in range(WARMUP):
        for g in forms:
            timed(g)
    ts = [[] for _ in forms]
    for _ in range(REPEATS):
        for i, g in enumerate(forms):
            ts[i].append(timed(g))
    print("-- the clustering alone, %d variables, %d clusters" % (n, n_clusters))
    for (what, batch, samples), t in zip(shapes, ts):
        found = data[what][1][0].cpu().numpy().view(BRANCH_INFO_DTYPE)["n_branches"]
        assert np.all(found == n_clusters), (what, found)
        line(what, t, batch * samples)


def main():
    if E.device_count() < 1:
        raise SystemExit("tools/branches_rate.py needs a HIP device")
    stream = torch.cuda.Stream()
    print("Solution branches (ezpz_system_solve_branches_device, ezpz_branch_cluster_device) on", torch.cuda.get_device_name(0))
    print("host clock around work that ends in a synchronise; %d warm-up run(s) of each form, then %d timed runs (host chain: %d), the forms"
          % (WARMUP, REPEATS, HOST_REPEATS))
    print("alternating; median (min .. max).  max_branches %d, eps 1e-5, rounds of %d samples after a first of %d." % (MAX_BRANCHES, CHUNK, FIRST_ROUND))
    big = R.chain(38)
    compare = np.zeros(big.n_vars, np.uint8)
    compare[4:10] = 1
    for name, f, half_width, mask in (("blocks(3), 18 variables", R.blocks(3), 3.0, None),
                                      ("chain(38), a connected sketch of 80 variables", big, 3.0, compare)):
        for samples in SAMPLES:
            run_case(name, f, half_width, mask, samples, stream)
    for n_clusters in (2, 8, 32):
        cluster_case(n_clusters, stream)


if __name__ == "__main__":
    main()
