"""N>1 path (sharded.py): world_size-2/3 gloo runs.  CPU: the oracle stands in for the GPU engine
and checks the host logic; GPU: the product engine, all ranks on the box's one GPU."""
import importlib
import json
import os
import random
import shutil
import subprocess
import sys

import pytest

from __graft_entry__ import ROOT, load_package


def free_port():
    """a port nobody listens on right now (two test sessions on one box must not share a rendezvous port)"""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_world(engine, world, n_bases, k, tmp_path, port, mode="gather", backend="gloo", parts=3):
    port = free_port()                      # (the callers' fixed numbers are kept only as labels)
    out = tmp_path / f"res_{engine}_{mode}_{world}_{n_bases}_{k}_{backend}_{parts}.json"
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", SHARD_BACKEND=backend, SHARD_PARTS=str(parts))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_sharded_worker.py"),
                                       engine, str(n_bases), str(k), str(out), mode], env=env))
    for p in procs:
        assert p.wait(timeout=600) == 0
    return json.loads(out.read_text())


def test_shard_ranges_cover_exactly_once():
    pkg = load_package()
    sh = importlib.import_module(pkg.__name__ + ".shard_math")
    for n, k, w in [(1000, 31, 2), (1000, 31, 8), (64, 32, 3), (31, 31, 4), (30, 31, 2), (3_000_000_000, 31, 8)]:
        r = sh.shard_ranges(n, k, w)
        n_kmers = max(n - k + 1, 0)
        assert sum(x[1] for x in r) == n_kmers
        pos = 0
        for first, cnt, lo, hi in r:
            assert first == pos and lo % 32 == 0
            if cnt:
                assert hi == min(first + cnt + k - 1, n)      # k-1 base halo, clipped at the end
            pos += cnt


def test_word_chunks_cover_the_sequence():
    pkg = load_package()
    sh = importlib.import_module(pkg.__name__ + ".shard_math")
    for n, w in [(1000, 2), (1000, 8), (64, 3), (31, 4), (3_000_000_000, 8), (33, 5)]:
        per, chunks = sh.word_chunks(n, w)
        assert sum(c[1] for c in chunks) == n
        pos = 0
        for lo, nb in chunks:
            assert nb == 0 or lo * 32 == pos
            assert nb <= per * 32
            pos += nb


@pytest.mark.parametrize("mode", ["gather", "keys"])
@pytest.mark.parametrize("world,n_bases,k", [(2, 200_000, 31), (3, 100_001, 21), (2, 5000, 8)])
def test_sharded_count_gloo_oracle_engine(tmp_path, world, n_bases, k, mode):
    res = run_world("oracle", world, n_bases, k, tmp_path, 29511 + world + (10 if mode == "keys" else 0), mode)
    assert res["ok"] and res["sorted"], res


def test_bucket_owner_ranges_cover_exactly_once():
    pkg = load_package()
    sh = importlib.import_module(pkg.__name__ + ".shard_math")
    for nb, w in [(64, 8), (56, 8), (7, 2), (7, 3), (1, 4), (128, 6), (3, 8)]:
        r = sh.bucket_owner_ranges(nb, w)
        assert r[0][0] == 0 and r[-1][1] == nb
        for (lo, hi), (lo2, _) in zip(r, r[1:]):
            assert lo <= hi == lo2
        for b in range(nb):
            o = (b * w) // nb
            assert r[o][0] <= b < r[o][1]


def test_bucket_owner_ranges_weighted():
    pkg = load_package()
    sh = importlib.import_module(pkg.__name__ + ".shard_math")
    import random
    rnd = random.Random(5)
    for nb, w in [(68, 8), (64, 8), (7, 3), (1, 4), (128, 6), (3, 8), (68, 1)]:
        for trial in range(20):
            weights = [rnd.randint(0, 1000) if rnd.random() < 0.9 else 0 for _ in range(nb)]
            r = sh.bucket_owner_ranges_weighted(weights, w)
            assert len(r) == w and r[0][0] == 0 and r[-1][1] == nb
            for (lo, hi), (lo2, _) in zip(r, r[1:]):
                assert lo <= hi == lo2
            tot = sum(weights)
            if tot and w > 1 and nb >= 4 * w:
                share = [sum(weights[lo:hi]) for lo, hi in r]
                assert max(share) <= tot / w + max(weights), (nb, w, share)     # within one bucket of the even share
    assert sh.bucket_owner_ranges_weighted([0] * 10, 3) == sh.bucket_owner_ranges(10, 3)


# ------------------------------------------------------------------ multi_math.hpp (the one-process path's arithmetic) on the host

def build_plan_check(tmp_path, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / name)
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", *extra, "-I",
                           os.path.join(ROOT, "dna-sequences-pg-extension_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "multi_plan_check.cpp"), "-o", exe])
    return exe


SANITIZERS = ["-g", "-Xarch_host", "-fsanitize=address,undefined"]


@pytest.fixture(scope="module", params=[[], SANITIZERS], ids=["plain", "sanitizers"])
def plan_check(request, tmp_path_factory):
    """tests/host/multi_plan_check.cpp as a stand-alone host program; the second build has AddressSanitizer and
    UndefinedBehaviorSanitizer on its host code.  -> run(mode_args, text_in) -> the lines it printed"""
    exe = build_plan_check(tmp_path_factory.mktemp("multi_plan"), "multi_plan_check", request.param)

    def run(args, text_in):
        r = subprocess.run([exe, *args], input=text_in, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


PLAN_KINDS = ("uniform", "sparse", "ones", "spike", "wide")


def plan_weights(kind, nb, rnd):
    """weights below 2^40 (1024 of them sum below 2^50): every number the two rules compare is exact in a double"""
    if kind == "uniform":
        w = [rnd.randint(1, 1000) for _ in range(nb)]
    elif kind == "sparse":
        w = [rnd.randint(1, 1000) if rnd.random() < 0.1 else 0 for _ in range(nb)]
        w[rnd.randrange(nb)] = rnd.randint(1, 1000)             # never all zero
    elif kind == "ones":
        w = [1] * nb
    elif kind == "spike":
        w = [1] * nb
        w[rnd.randrange(nb)] = 1000 * nb
    else:
        w = [rnd.randrange(1 << 40) for _ in range(nb)]
    return w


def plan_sweep():
    """(W, P, weights): the five kinds at every W, P and bucket count, then nothing to weigh at every W, P and bucket count"""
    rnd = random.Random(0x6D706C616E)
    cases = [(W, P, plan_weights(kind, nb, rnd)) for W in (1, 2, 3, 8) for P in (1, 2, 3, 8) for nb in (1, 2, 5, 17, 136, 1024)
             for kind in PLAN_KINDS]
    assert all(sum(w) > 0 for _, _, w in cases)
    return cases + [(W, P, [0] * nb) for W in (1, 2, 3, 8) for P in (1, 2, 3, 8) for nb in (1, 2, 5, 17, 136, 1024)]


def test_exchange_plan_matches_shard_math(plan_check):
    """exchange_cuts of multi_math.hpp (what dnagpu_count_multi_unordered plans its record exchange with) against
    shard_math.py (what the process-per-GPU path plans with): bucket_owner_ranges_weighted, then bucket_group_cuts on every
    owner's range -- one rule, cut for cut.  With nothing to weigh: the even W * P split.  And the landing layout of every
    group: its record total, boff[] the exclusive prefix of blen[], blen[] the weights of its buckets and 0 elsewhere."""
    pkg = load_package()
    sh = importlib.import_module(pkg.__name__ + ".shard_math")
    cases = plan_sweep()
    out = plan_check([], "".join(f"{W} {P} {len(w)} {' '.join(map(str, w))}\n" for W, P, w in cases))
    assert len(out) == 3 * len(cases)
    for i, (W, P, w) in enumerate(cases):
        nb, what = len(w), f"W={W} P={P} nb={len(w)} case {i}"
        tag, *cuts = out[3 * i].split()
        cuts = [int(c) for c in cuts]
        assert tag == "cuts" and len(cuts) == W * P + 1, what
        if sum(w):
            want = []
            owners = sh.bucket_owner_ranges_weighted(w, W)
            for o, (lo, hi) in enumerate(owners):
                g = sh.bucket_group_cuts(w, lo, hi, P)
                assert len(g) == P + 1 and g[0] == lo and g[-1] == hi == (owners[o + 1][0] if o + 1 < W else nb), what
                want += g[:-1]
            want.append(nb)
        else:
            want = [-(-j * nb // (W * P)) for j in range(W * P)] + [nb]
        assert cuts == want, what
        assert cuts[0] == 0 and cuts[-1] == nb and all(a <= b for a, b in zip(cuts, cuts[1:])), what
        tag, *groups = out[3 * i + 1].split()
        groups = [tuple(int(v) for v in g.split(":")) for g in groups]
        assert tag == "groups" and len(groups) == W * P, what
        assert groups == [(sum(w[a:b]),) * 2 for a, b in zip(cuts, cuts[1:])], what
        assert sum(g[0] for g in groups) == sum(w), what
        tag, *layout, rest = out[3 * i + 2].split()
        assert tag == "layout" and rest == "rest=0" and len(layout) == nb, what
        want_layout = [f"{w[b]}:{sum(w[a:b])}" for a, e in zip(cuts, cuts[1:]) for b in range(a, e)]
        assert layout == want_layout, what


def test_rank_rows_tile_the_window(plan_check):
    """rank_rows of multi_math.hpp (the rows a rank sweeps in dnagpu_count_multi's table path and in the record exchange)
    against word_chunks: the ranks' rows tile the window exactly once, a rank's rows are the window's rows that start in its
    chunk, and the neighbour's first word is needed exactly when a rank with rows has a chunk that ends before the sequence"""
    pkg = load_package()
    sh = importlib.import_module(pkg.__name__ + ".shard_math")
    cases = []
    for n in (1, 31, 32, 33, 200, 100_001):
        for W in (1, 2, 3, 8):
            per, chunks = sh.word_chunks(n, W)
            for k in (21, 31):
                rows = max(n - k + 1, 0)
                windows = {(0, rows), (rows // 3, rows // 3), (min(1, rows), max(rows - 2, 0)), (rows, 0)}
                for r in range(W):                          # inside one rank's chunk; up to its last row; across its end
                    lo = chunks[r][0] * 32
                    for first, count in ((lo + 3, 10), (lo + 3, per * 32 - 3), (lo + per * 16, per * 32)):
                        if first + count <= rows:
                            windows.add((first, count))
                cases += [(n, W, per, chunks, first, count) for first, count in sorted(windows)]
    out = plan_check(["rows"], "".join(f"{(n + 31) // 32} {per} {W} {first} {count}\n" for n, W, per, _, first, count in cases))
    assert len(out) == len(cases)
    some_halo = some_empty = False
    for line, (n, W, per, chunks, first, count) in zip(out, cases):
        what = f"n={n} W={W} rows [{first}, {first + count})"
        got = [tuple(int(v) for v in f.split(":")) for f in line.split()]
        assert len(got) == W, what
        pos = first
        for (w_hi, row_lo, row_hi, halo), (w_lo, nbases) in zip(got, chunks):
            chunk_end = w_lo * 32 + nbases                  # first base behind the chunk
            assert w_hi == (chunk_end + 31) // 32, what
            if row_hi > row_lo:
                assert row_lo == pos == max(first, w_lo * 32) and row_hi == min(first + count, w_hi * 32), what
                pos = row_hi
            else:
                assert min(first + count, w_hi * 32) <= max(first, w_lo * 32), what     # no row of the window starts here
                some_empty = True
            assert halo == (1 if row_hi > row_lo and chunk_end < n else 0), what
            some_halo |= bool(halo)
        assert pos == first + count, what
    assert some_halo and some_empty


@pytest.mark.parametrize("world,n_bases,k,parts", [(2, 200_000, 31, 3), (3, 100_001, 25, 3), (2, 5000, 23, 2), (3, 100_001, 25, 1),
                                                   (2, 200_000, 31, 1)])
def test_sharded_records_gloo_oracle_engine(tmp_path, world, n_bases, k, parts):
    """the record exchange's host logic (bucket owners, bucket groups, split sizes, piece boundaries) with the oracle
    standing in: one all-to-all (parts = 1) and the pipelined point-to-point rounds (parts > 1)"""
    res = run_world("oracle", world, n_bases, k, tmp_path, 0, "records", parts=parts)
    assert res["ok"] and res["sorted"], res


@pytest.mark.gpu
@pytest.mark.parametrize("world,n_bases,k,parts", [(2, 3_000_000, 31, 3), (3, 1_000_003, 27, 1), (2, 70_000, 23, 2), (1, 6_000_000, 31, 1),
                                                   (2, 3_000_000, 31, 1)])
def test_sharded_records_gloo_gpu_engine(tmp_path, world, n_bases, k, parts):
    """count_sharded_exchange_records with the product engine: every rank cuts the records of its own rows
    (dnagpu_sk_records), the buckets travel to their owners, the owners count them (dnagpu_count_records)"""
    res = run_world("gpu", world, n_bases, k, tmp_path, 0, "records", parts=parts)
    assert res["ok"] and res["sorted"], res


@pytest.mark.gpu
def test_sharded_records_rccl_one_rank(tmp_path):
    for parts in (1, 3):
        res = run_world("gpu", 1, 2_000_000, 31, tmp_path, 0, "records", backend="nccl", parts=parts)
        assert res["ok"] and res["sorted"], res


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gather", "keys"])
@pytest.mark.parametrize("world,n_bases,k", [(2, 3_000_000, 31), (3, 1_000_003, 21), (2, 70_000, 4)])
def test_sharded_count_gloo_gpu_engine(tmp_path, world, n_bases, k, mode):
    if mode == "keys" and k < 6:
        pytest.skip("the key-exchange variant needs 2k > 10 bits")
    res = run_world("gpu", world, n_bases, k, tmp_path, 29531 + world + (10 if mode == "keys" else 0), mode)
    assert res["ok"] and res["sorted"], res


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gather", "keys"])
def test_sharded_count_rccl_one_rank(tmp_path, mode):
    """The product backend (nccl = RCCL) with the collectives forced at world size 1: device tensors, the
    library's stream and torch's stream meet the way they do on the 8-GPU node (a one-GPU box cannot
    host two RCCL ranks)."""
    res = run_world("gpu", 1, 2_000_000, 31, tmp_path, 29561 + (1 if mode == "keys" else 0), mode, backend="nccl")
    assert res["ok"] and res["sorted"], res


@pytest.mark.gpu
def test_pool_buffer_on_another_stream(tmp_path):
    """include/dnagpu.h's stream rule for pooled buffers, exercised from a non-default torch stream (own process: torch
    brings its own ROCm runtime)"""
    out = tmp_path / "stream.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_stream_worker.py"), str(out)],
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), timeout=600)
    assert p.returncode == 0
    res = json.loads(out.read_text())
    assert res["ok"], res
