"""Time the full model's data-parallel training step (train.train_step with a distributed.GradSync) on N GPUs.

  python tools/time_train_ddp.py [--gpus 1,2,4,8] [--force] [--graphs 4096] [--steps 10] [--warmup 3] [--out profiles/<name>.json]
  python tools/time_train_ddp.py --build-plain-loads

Ranks are started the way bench.py --gpus N starts them -- fresh child processes of this one, which never touches the GPU itself
-- each under a `timeout` of its own (--limit seconds), at most 8; rank, world and port travel on the command line and the
environment is passed on as it is.  The workload is tools/time_train_full.py's (synthetic.make_full_workload, 4096 questions of
12 tokens, the model in train() mode), cut by graph with distributed.shard_workload; every rank trains its share with
optim.Adam(lr=1e-4, max_grad_norm=2.0, grad_sync=sync).  --force runs pack() and reduce() on one rank too (a one-rank RCCL group).

Per rank count, rank 0 reports: ms per step (host clock around --steps synchronised steps); HIP-event times of pack() and of
reduce() inside the steps of a second window; pack() alone beside a torch copy_ of the same bytes, and -- when
--build-plain-loads made tools/_build/libisg_hip_plain_loads.so here -- isg_mt_pack with ordinary source loads on the same table;
params_in_sync() after the run; optim.LAUNCHES["table_copies"].  With one rank the same step without a sync is timed as well.
A rank count whose ranks do not all end with status 0 ends the run: nothing more is started."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_LIB = os.path.join(ROOT, "tools", "_build", "libisg_hip_plain_loads.so")


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", default="1", help="rank counts, comma-separated; at most 8 each")
    ap.add_argument("--force", action="store_true", help="pack and all-reduce on one rank too")
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds a rank may run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--build-plain-loads", action="store_true")
    ap.add_argument("--rank", type=int, default=None)
    ap.add_argument("--world", type=int, default=None)
    ap.add_argument("--port", type=int, default=None)
    a = ap.parse_args(argv)
    a.counts = [int(v) for v in str(a.gpus).split(",")]
    if any(n < 1 or n > 8 for n in a.counts):
        ap.error("--gpus: 1 to 8 ranks")
    return a


def build_plain_loads():
    """The library once more with csrc/isg_dist.hip compiled -DISG_PACK_PLAIN_LOADS; every other object is the library's own."""
    sys.path.insert(0, ROOT)
    import glob
    import __graft_entry__ as ge
    ge.build()
    src = os.path.join(ge.CSRC, "isg_dist.hip")
    objs = sorted(o for o in glob.glob(os.path.join(ge.CSRC, "_obj", "*.o")) if not o.endswith(".strict.o"))
    os.makedirs(os.path.dirname(PLAIN_LIB), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    plain = os.path.join(os.path.dirname(PLAIN_LIB), "isg_dist.plain_loads.o")
    subprocess.check_call([hipcc, *ge.flags_for(src), "-DISG_PACK_PLAIN_LOADS", "-c", src, "-o", plain], cwd=ge.CSRC)
    link = [plain if os.path.basename(o) == "isg_dist.o" else o for o in objs]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", *link, "-o", PLAIN_LIB], cwd=ge.CSRC)
    print(f"[time_train_ddp] built {PLAIN_LIB}")


def free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(a, world: int):
    """Start `world` ranks, return rank 0's result; None when a rank failed."""
    port = free_port()
    base = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--world", str(world), "--port", str(port),
            "--graphs", str(a.graphs), "--steps", str(a.steps), "--warmup", str(a.warmup)] + (["--force"] if a.force else [])
    procs = [subprocess.Popen(base + ["--rank", str(r)], stdout=subprocess.PIPE if r == 0 else sys.stderr, text=True)
             for r in range(world)]
    result = None
    for line in procs[0].stdout:
        if line.startswith('{"ranks"'):
            result = json.loads(line)
        else:
            sys.stderr.write(line)
    codes = [p.wait() for p in procs]
    if any(codes):
        print(f"[time_train_ddp] {world} ranks ended with {codes}", file=sys.stderr)
        return None
    return result


def events(fn, n):
    """Mean HIP-event time of fn() in us over n calls behind two warm ones."""
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1) / n * 1e3, 1)


def rank_main(a):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import isubgvqa_amd  # noqa: F401
    from isubgvqa_amd import distributed, ops, optim, synthetic, train
    from isubgvqa_amd.models import build_model
    rank, world = a.rank, a.world
    assert torch.cuda.is_available() and torch.cuda.device_count() >= world, \
        f"{world} ranks need {world} GPUs, this box shows {torch.cuda.device_count()}"
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    grouped = world > 1 or a.force
    if grouped:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{a.port}", rank=rank, world_size=world, device_id=dev)
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(), None).to(dev).train()
    wl = distributed.shard_workload(synthetic.make_full_workload(a.graphs), rank, world).to(dev)
    rows = wl.questions.size(0)
    target = torch.randint(0, 1842, (a.graphs,), generator=torch.Generator().manual_seed(1))[rank * ((a.graphs + world - 1) // world):][:rows].to(dev)
    inputs = dict(node_embeddings=wl.x, edge_index=wl.edge_index, edge_embeddings=wl.edge_attr, batch=wl.batch, questions=wl.questions,
                  qsts_att_mask=wl.att_mask, return_masks=True, scene_graphs=wl.scene_graphs())
    sync = distributed.GradSync(model.named_parameters(), force=a.force)
    sync.broadcast_params()
    opt = optim.Adam(model.parameters(), lr=1e-4, max_grad_norm=2.0, grad_sync=sync)
    meters = train.Meters(dev)
    seed = [1000]

    def steps(n, optimizer=opt, s=sync):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            seed[0] += 1
            train.train_step(model, optimizer, inputs, target, meters, seed=seed[0], sync=s)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    steps(a.warmup)
    res = {"ranks": world, "rows_per_rank": rows, "sync_active": sync.active, "device": torch.cuda.get_device_name(rank),
           "gpus_visible": torch.cuda.device_count(),
           "parameters": sum(p.numel() for p in model.parameters())}
    res["ms_per_step"] = round(steps(a.steps), 3)
    if sync.active:
        # a second window with HIP events around the two calls (the all-reduce runs on the communicator's stream; the current
        # stream waits for it before the second event)
        spans = {"pack": [], "reduce": []}
        plain = {k: getattr(sync, k) for k in spans}

        def timed(name):
            def call(*args, **kw):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                plain[name](*args, **kw)
                t1.record()
                spans[name].append((t0, t1))
            return call

        for name in spans:
            setattr(sync, name, timed(name))
        res["ms_per_step_with_events"] = round(steps(a.steps), 3)
        for name in spans:
            delattr(sync, name)
            us = [t0.elapsed_time(t1) * 1e3 for t0, t1 in spans[name]]
            res[f"{name}_us"] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}
        res["bucket_bytes"] = sync.bucket.numel() * 4
        res["tensors_in_set"] = len(sync.members)
        # pack() alone (the gradients of the last step are still there) beside a copy_ of the same bytes
        src, dst = torch.randn(sync.bucket.numel(), device=dev), torch.empty(sync.bucket.numel(), device=dev)
        res["pack_alone_us"] = events(sync.pack, 20)
        res["copy_same_bytes_us"] = events(lambda: dst.copy_(src), 20)
        res["pack_over_copy"] = round(res["pack_alone_us"] / res["copy_same_bytes_us"], 3)
        if os.path.exists(PLAIN_LIB):
            import ctypes
            from isubgvqa_amd import _lib, _lib_dist
            other = _lib.bind(ctypes.CDLL(PLAIN_LIB), _lib_dist.SIGNATURES)
            T, base = len(sync.members), sync._table.data_ptr()
            call = lambda lib: lib.isg_mt_pack(base, base + 8 * T, base + 16 * T, base + 24 * T, T, sync._chunks, 1.0 / world, 0, ops._stream())
            assert call(other) == 0
            rounds = [(events(lambda: call(_lib_dist.load()), 20), events(lambda: call(other), 20)) for _ in range(3)]
            res["isg_mt_pack_non_temporal_loads_us"] = [r[0] for r in rounds]
            res["isg_mt_pack_plain_loads_us"] = [r[1] for r in rounds]
        del src, dst
    res["params_in_sync"] = int(sync.params_in_sync()) if grouped else None
    res["table_copies"] = optim.LAUNCHES["table_copies"]
    res["src_copies"] = distributed.LAUNCHES["src_copies"]
    res["meters"] = meters.report(dist.group.WORLD if grouped else None)
    if world == 1:                                  # the same step without a sync, from p.grad
        stock = optim.Adam(model.parameters(), lr=1e-4, max_grad_norm=2.0)
        steps(a.warmup, stock, None)
        res["ms_per_step_without_sync"] = round(steps(a.steps, stock, None), 3)
    res["max_memory_allocated_MiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    if grouped:
        dist.barrier()
        torch.cuda.synchronize()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(res), flush=True)


def main():
    a = parse()
    if a.build_plain_loads:
        return build_plain_loads()
    if a.rank is not None:
        return rank_main(a)
    out = {"workload": f"full ISubGVQA model, {a.graphs} questions in all, cut by graph over the ranks, train() mode; a whole step: "
                       "forward, loss, backward, pack, all-reduce, clip at 2.0, Adam",
           "method": f"{a.warmup} warm steps, then {a.steps} steps between two device synchronisations (host clock); pack / reduce: "
                     "HIP events around the calls in a second window of the same length", "per_rank_count": {}}
    status = 0
    for world in a.counts:
        res = launch(a, world)
        if res is None:
            status = 1
            break
        out["per_rank_count"][str(world)] = res
        print(json.dumps(res), flush=True)
    if a.out and out["per_rank_count"]:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
