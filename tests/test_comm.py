"""polr_bcast_build -- the path's one exchange step (RCCL inside the product library) -- on the one GPU of the test box:
a communicator of world size 1 exercises id creation, ncclCommInitRank, the metadata / buffer walk and ncclBroadcast
calls end to end; the receiving side (polr_ht_alloc_like + in-place buffer broadcast) is the same code the N > 1 run
uses and is covered by tests/test_gpu_build_routes.py::test_clone (export -> alloc_like -> buffer copies, the source closed,
every table kind against the numpy reference)."""
import numpy as np
import pytest

from buildside import _d2d
from polr_amd import capi, workloads


@pytest.mark.gpu
def test_bcast_build_world_of_one(gpu_ctx):
    wl = workloads.star_skew(n_fact=50_000)
    joins = capi.build_joins(gpu_ctx, wl)
    uid = capi.comm_unique_id()
    assert len(uid) == capi.COMM_ID_BYTES and any(uid)
    comm = capi.Comm(gpu_ctx, uid, 1, 0)
    total = 0
    for ht, _ in joins:
        meta, bufs = ht.export()
        same = comm.bcast_build(ht, root=0)
        assert same is ht
        total += sum(int(b[1]) for b in bufs)
    assert comm.bytes_broadcast() == total
    # the tables still probe as before
    cols = list(wl["probe"]["cols"].values())
    pipe = capi.Pipeline(gpu_ctx, cols, len(cols[0]), joins, workloads.default_paths(len(joins)))
    counts = pipe.probe_rounds([(0, len(cols[0]), 0, 0)])
    assert counts.sum() > 0
    pipe.close()
    comm.close()


@pytest.mark.gpu
def test_bcast_build_keeps_a_packed_composite_key(gpu_ctx):
    """the per-column [min, max] packing of a three-key table travels in the metadata blob"""
    import numpy as np
    rng = np.random.default_rng(5)
    bk = [rng.integers(-40, 40, 3000).astype(np.int32), rng.integers(0, 9, 3000).astype(np.uint8),
          rng.integers(100, 130, 3000).astype(np.int16)]
    ht = capi.HashTable.from_columns(gpu_ctx, bk, [])
    ht.finalize_hash()
    meta, bufs = ht.export()
    clone = capi.HashTable.alloc_like(gpu_ctx, meta)
    _m2, bufs2 = clone.export()
    for (src, n), (dst, n2) in zip(bufs, bufs2):
        assert n == n2
        if n:
            _d2d(dst, src, n)
    pick = rng.integers(0, 3000, 8000)
    pk = [b[pick].copy() for b in bk]
    pk[0][::5] += 1000  # out of range: no match
    counts = []
    for t in (ht, clone):
        pipe = capi.Pipeline(gpu_ctx, pk, 8000, [(t, [(-1, 0), (-1, 1), (-1, 2)])], [[0]])
        counts.append(int(pipe.probe_rounds([(0, 8000, 0, 0)]).sum()))
        pipe.close()
    assert counts[0] == counts[1] > 0


@pytest.mark.gpu
def test_bcast_build_failures_are_collective_world_of_one(gpu_ctx):
    """a root without a finalized table still runs the metadata broadcast (size 0) and returns an error -- no rank-local
    early return ahead of a collective; the communicator stays usable afterwards"""
    comm = capi.Comm(gpu_ctx, capi.comm_unique_id(), 1, 0)
    raw = capi.HashTable.from_columns(gpu_ctx, [np.arange(100, dtype=np.int32)], [])  # never finalized
    with pytest.raises(capi.PolrError) as e:
        comm.bcast_build(raw, root=0)
    assert "no finalized build side" in str(e.value)
    with pytest.raises(capi.PolrError):
        comm.bcast_build(None, root=0)
    assert comm.bytes_broadcast() == 0
    raw.finalize_hash()
    assert comm.bcast_build(raw, root=0) is raw and comm.bytes_broadcast() > 0
    comm.close()
    raw.close()


_TWO_RANK = r"""
import os, sys, json
import numpy as np
rank, world, port = int(sys.argv[1]), 2, sys.argv[2]
sys.path.insert(0, sys.argv[3]); sys.path.insert(0, sys.argv[4])
os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
import torch, torch.distributed as dist
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=world)
from polr_amd import capi, workloads
ctx = capi.Context(rank)
idt = torch.zeros(capi.COMM_ID_BYTES, dtype=torch.uint8)
if rank == 0:
    idt.copy_(torch.tensor(list(capi.comm_unique_id()), dtype=torch.uint8))
dist.broadcast(idt, 0)
comm = capi.Comm(ctx, bytes(idt.numpy().tobytes()), world, rank)
wl = workloads.star_skew(n_fact=50_000)
joins = capi.build_joins(ctx, wl) if rank == 0 else None
got = []
for x, j in enumerate(wl["joins"]):
    ht = comm.bcast_build(joins[x][0] if rank == 0 else None, root=0)
    got.append((ht, j["key_src"]))
# a failing root: every rank gets an error out of the same call, nobody hangs
raw = capi.HashTable.from_columns(ctx, [np.arange(10, dtype=np.int32)], []) if rank == 0 else None
failed = False
try:
    comm.bcast_build(raw, root=0)
except capi.PolrError:
    failed = True
cols = list(wl["probe"]["cols"].values())
pipe = capi.Pipeline(ctx, cols, len(cols[0]), got, workloads.default_paths(len(got)))
counts = pipe.probe_rounds([(0, len(cols[0]), 0, 0)])
print(json.dumps({"rank": rank, "failed": failed, "counts": counts.tolist(), "bytes": comm.bytes_broadcast()}), flush=True)
dist.barrier()
"""


@pytest.mark.gpu
def test_bcast_build_two_ranks_over_rccl(tmp_path):
    """world size 2 over RCCL: rank 1's received tables probe like rank 0's own.  Needs two GPUs (the driver's 8-GPU node;
    skipped on the one-GPU test boxes -- where it has never run, the N > 1 receive path is UNVERIFIED ON HARDWARE)"""
    import json
    import os
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "two_rank.py"
    script.write_text(_TWO_RANK)
    port = str(29500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), port, os.path.join(root, "duckdb-polr_amd", "python"), root],
                              stdout=subprocess.PIPE, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        assert p.returncode == 0
        outs.append(json.loads(o.strip().splitlines()[-1]))
    assert outs[0]["counts"] == outs[1]["counts"] and outs[0]["failed"] and outs[1]["failed"]
    assert outs[0]["bytes"] == outs[1]["bytes"] > 0


def test_comm_api_rejects_null_arguments():
    L = capi.load()
    assert L.polr_comm_get_unique_id(None) == capi.E_INVALID
    assert L.polr_bcast_build(None, None, 0, None) == capi.E_INVALID
