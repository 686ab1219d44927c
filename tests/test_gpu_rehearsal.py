"""The multi-rank path of bench.py on ONE GPU.  Kept in its own file, collected after the kernel parity tests: these tests start
subprocesses (torch.distributed.run), and a rendezvous hiccup here must not hide the kernel parity tests when the suite runs with -x.

  * REHEARSAL (PVS_BENCH_BACKEND=gloo): 2-4 ranks share this GPU, collectives staged through the host -- everything of the N > 1
    run but the RCCL transport; every rank asserts that its lists equal the plain single-GPU ranking bit for bit.
  * ONE-rank RCCL self-check (PVS_BENCH_FORCE_DIST=1): the same code path on the measured transport -- the RCCL communicator
    behind the C-ABI (pvs_comm_*), on its own stream, ordered by events against the compute stream."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def _run_bench(ranks, env_extra, extra_args, timeout=900):
    from conftest import REPO
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    if "PVS_BENCH_BACKEND" not in env_extra:
        env.pop("PVS_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(REPO, "bench.py"), "--gpus", str(ranks), "--full", "--no-cpu-baseline"] + extra_args
    r = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return r, line


@pytest.mark.parametrize("ranks,retrieval", [(2, "exact"), (3, "exact"), (4, "exact"), (2, "filtered")])
def test_multi_rank_bench_rehearsal(ranks, retrieval):
    """configs[1] (8189-image generator, reduced): image sharding, exchange, block-pair scoring (or the filtered retrieval against
    the gathered corpus), all-to-all of candidate lists, merge."""
    r, line = _run_bench(ranks, {"PVS_BENCH_BACKEND": "gloo"}, ["--steps", "1", "--warmup", "1", "--images", "1030", "--retrieval", retrieval])
    assert r.stderr.count("identical to the single-GPU ranking") == ranks, r.stderr[-3000:]
    assert line["n_gpus"] == ranks and "REHEARSAL" in line["backend"] and line["retrieval"] == retrieval


@pytest.mark.parametrize("ranks,retrieval", [(2, "exact"), (3, "filtered"), (2, "f16")])
def test_sharded_corpus1m_rehearsal(ranks, retrieval):
    """configs[3] / configs[4] (images x 512 uint8 descriptors generated and encoded chunk by chunk, every rank its block; all-vs-all
    top-10), reduced to 20000 images: exact and filtered lists bit-identical to the plain ranking on every rank; fp16 lists
    gathered as fp16 blocks, self-retrieval checked."""
    r, line = _run_bench(ranks, {"PVS_BENCH_BACKEND": "gloo"},
                         ["--workload", "corpus1m", "--steps", "1", "--warmup", "0", "--images", "20000", "--retrieval", retrieval])
    if retrieval != "f16":
        assert r.stderr.count("identical to the single-GPU ranking") == ranks, r.stderr[-3000:]
    assert line["n_gpus"] == ranks and line["config"]["images"] == 20000 and "configs[3]" in line["config"]["workload"]


@pytest.mark.parametrize("workload,retrieval", [("config2", "exact"), ("config2", "filtered"), ("corpus1m", "exact"), ("corpus1m", "f16")])
def test_one_rank_rccl_self_check(workload, retrieval):
    """One rank on RCCL through pvs_comm_init / pvs_allgather_dev / pvs_alltoall_dev: exchange stream + event ordering, the
    all-gather overlapped with the (r, r) block, the list all-to-all -- against the plain single-GPU retrieval."""
    args = ["--steps", "2", "--warmup", "1", "--retrieval", retrieval, "--workload", workload,
            "--images", "1030" if workload == "config2" else "20000"]
    r, line = _run_bench(1, {"PVS_BENCH_FORCE_DIST": "1"}, args)
    if retrieval != "f16":
        assert r.stderr.count("identical to the single-GPU ranking") == 1, r.stderr[-3000:]
    else:
        assert line["self_check"]["fp16_recall_at_k_vs_exact_f32"] >= 0.99
    assert "RCCL self-check" in line["backend"] and "RCCL behind the C-ABI" in line["exchange"]


@pytest.mark.parametrize("ranks,env", [(3, {"PVS_BENCH_BACKEND": "gloo"}), (1, {"PVS_BENCH_FORCE_DIST": "1"})], ids=["gloo-3-ranks", "rccl-1-rank"])
def test_bounded_query_block_travels_instead_of_the_database(ranks, env):
    """The N > 1 default (a bounded query block over a sharded corpus): the ranks all-gather their QUERY blocks, rank all of them
    against their own database block, return k candidates per query by all-to-all and merge -- instead of all-gathering the
    database.  20000 images, 3000 queries in all; recall@10 of every rank's lists against its exact fp32 ranking (asserted inside
    bench.py on every rank), self-retrieval first."""
    r, line = _run_bench(ranks, env, ["--workload", "corpus1m", "--steps", "1", "--warmup", "1", "--images", "20000", "--retrieval", "f16",
                                      "--total-queries", "3000"])
    assert line["exchange_plan"].startswith("queries travel") and line["queries_per_step"] == 3000 // ranks * ranks
    assert line["self_check"]["fp16_recall_at_k_vs_exact_f32"] >= 0.99


def test_corpus1m_single_gpu_filtered_equals_exact():
    """Single GPU, no launcher: the chunked corpus build + filtered retrieval, lists bit-identical to the all-pairs f32 GEMM."""
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--full", "--workload", "corpus1m", "--images", "30000", "--steps", "1",
                        "--warmup", "0", "--retrieval", "filtered", "--queries", "2048"], cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["self_check"]["lists_bit_identical_to_plain_exact_ranking"] is True and line["n_gpus"] == 1


@pytest.mark.parametrize("retrieval,qflag,nq", [("f16", "--total-queries", 4096), ("filtered", "--queries", 2048), ("filtered", "--queries", 2)])
def test_corpus1m_at_its_stated_size_on_one_gpu(retrieval, qflag, nq):
    """BASELINE configs[3] / configs[4] at their stated size, on the one GPU a test has: 1,000,000 images x 512 uint8 descriptors
    generated and encoded chunk by chunk (202 GB resident), then a query block ranked against all 10^6 rows.  f16 = configs[4]'s
    fp16 MFMA similarity (recall@10 of 256 sampled queries against their exact fp32 lists); filtered = the exact lists through
    the fp16 prefilter + fp32 re-scoring, bit-identical on 256 sampled queries to the all-pairs fp32 GEMM -- and, with two queries, to the
    dense one-pass row kernel over all 10^6 rows (what a single query against a resident index takes).  Size-independent
    properties at full size: every query retrieves itself first with score 1 (asserted inside bench.py for both paths)."""
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--full", "--workload", "corpus1m", "--retrieval", retrieval,
                        qflag, str(nq), "--steps", "1", "--warmup", "0", "--no-cpu-baseline"], cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["config"]["images"] == 1000000 and line["queries_per_step"] == nq and line["n_gpus"] == 1
    if retrieval == "f16":
        assert line["self_check"]["fp16_recall_at_k_vs_exact_f32"] >= 0.99 and line["self_check"]["queries_checked"] == 256
    else:
        assert line["self_check"]["lists_bit_identical_to_plain_exact_ranking"] is True


def test_bench_starts_its_own_ranks_when_typed_without_a_launcher():
    """Literally `python3 bench.py --gpus 2 ...` (the form the driver types): the parent never touches the GPU, starts the two
    ranks as fresh processes through torch.distributed.run on 127.0.0.1 and relays rank 0's line.  With no workload flag the
    N > 1 default is BASELINE configs[3]/[4] (1M-image corpus generator, fp16 exchange and retrieval, a bounded query block
    shared out over the ranks); reduced here to 20000 images.  gloo REHEARSAL transport (two ranks on one GPU)."""
    from conftest import REPO
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PVS_BENCH_BACKEND="gloo")
    for k_ in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k_, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--full", "--steps", "1", "--warmup", "0", "--images", "20000",
                        "--total-queries", "4096"], env=env, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and "configs[3]/[4]" in line["config"]["workload"] and line["retrieval"] == "f16"
    assert line["queries_per_step"] == 4096 and line["scaling"] == "strong"
    assert line["self_check"]["fp16_recall_at_k_vs_exact_f32"] >= 0.99
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(line["roofline"])


def test_one_rank_rccl_point_to_point_and_collectives_without_torch():
    """pvs_sendrecv_dev (the neighbour exchange's primitive), pvs_alltoall_dev, pvs_allgather_dev, pvs_allreduce_max_f64 on a
    ONE-rank RCCL communicator behind the C-ABI, no torch in the process path: a self send / receive moves the bytes, a failing
    call inside a group leaves the communicator usable."""
    import numpy as np
    import pvsim
    from pvsim import distributed as pd
    ctx = pvsim.Context(0)
    comm = pd.RcclComm(ctx, 1, 0, pd.new_unique_id())
    try:
        src = np.arange(4096, dtype=np.float32)
        a, b, c = ctx.buffer(src.nbytes).upload(src), ctx.buffer(src.nbytes).fill_bytes(0), ctx.buffer(src.nbytes).fill_bytes(0)
        comm.send_recv([(0, a.ptr, src.nbytes, b.ptr, src.nbytes)])
        comm.all_to_all(c.ptr, a.ptr, src.nbytes)
        ctx.sync()
        assert np.array_equal(b.download(src.shape, np.float32), src)
        assert np.array_equal(c.download(src.shape, np.float32), src)
        with pytest.raises(ValueError):
            comm.send_recv([(3, a.ptr, 16, b.ptr, 16)])           # peer out of range: rejected before the group opens
        d = ctx.buffer(src.nbytes).fill_bytes(0)
        comm.all_gather(a.ptr, d.ptr, src.nbytes)                  # the communicator still works
        assert comm.max_over_ranks([1.5, -2.0]).tolist() == [1.5, -2.0]
        assert np.array_equal(d.download(src.shape, np.float32), src)
    finally:
        comm.close()
        ctx.close()
        comm.close()                                               # closing after the context is a no-op, not a use after free


def test_sharded_index_search_on_a_one_rank_rccl_communicator():
    """ShardedVLADIndex.search (a block of queries against the sharded index; the queries travel, the index stays): the whole
    path -- query all-gather, per-block ranking with global indices, candidate all-to-all, merge -- on a one-rank RCCL
    communicator, no torch object anywhere; lists bit-identical to the all-vs-all topk() rows of the same images."""
    import numpy as np
    import pvsim
    from conftest import REPO
    from pvsim import distributed as pd, synth, pack_descriptors
    from pvsim.engine import DESC_U8_ROOTSIFT
    tables = np.load(os.path.join(REPO, "tests", "golden", "tables_k256_d128.npz"), allow_pickle=False)
    ctx, ctx_x = pvsim.Context(0), pvsim.Context(0)         # compute stream, exchange stream (ordered by pvs_stream_wait inside the index)
    comm = pd.RcclComm(ctx_x, 1, 0, pd.new_unique_id())
    try:
        rng = np.random.default_rng(5)
        imgs = [synth.sift_like(int(n), rng).astype(np.uint8) for n in rng.integers(40, 300, size=41)]
        packed, off = pack_descriptors(imgs, 128, np.uint8)
        cb = ctx.codebook(tables["centroids"])
        pool = pd.DevicePool(ctx)
        d_x = pool.empty(packed.shape, "uint8").upload(packed)
        d_off = pool.empty(off.shape, "int64").upload(off)
        index = pd.ShardedVLADIndex(ctx, cb, len(imgs), comm)
        index.encode_local(d_x.ptr, DESC_U8_ROOTSIFT, d_off.ptr, int(off[-1]))
        index.exchange()
        idx_all, val_all = index.topk(5)
        for _ in range(2):                                   # the second call reuses the pool's blocks
            idx, val = index.search(index.enc_loc[:9], index.inv_loc[:9], 5)
            assert np.array_equal(idx, idx_all[:9]) and np.array_equal(val.view(np.uint32), val_all[:9].view(np.uint32))
        pool.close()
    finally:
        comm.close()
        ctx_x.close()
        ctx.close()
