"""Single-node data parallelism: one process per GPU, gradient all-reduce over RCCL/xGMI overlapped with backward.

The reference has no multi-GPU path at all; this is the new capability `north_star` asks for.
Partitioning: every rank holds a full weight replica (same seed), takes its own 16 tiles of the global batch
and normalises BatchNorm over them (plain DP, per-replica BN).  The only exchange is ONE sum-all-reduce of the
flat fp32 gradient arena per step, cut into buckets that are contiguous arena ranges.  Weight gradients land in
the arena in reverse layer order during the backward sweep, so bucket k is complete as soon as the sweep has
passed the first node owning parameters in it; it is then handed to RCCL on a communication stream behind an
event on the compute stream, while backward continues.  The 1/world scaling is folded into the Adam kernel
(`grad_scale`), so no extra pass touches the gradients.  The training loss and the four confusion counts are
summed over the ranks as well (metrics of the GLOBAL batch), BatchNorm moving statistics are averaged when a
checkpoint is written, and only rank 0 writes it.

Two transports behind one interface (`comm=`):
  "sg"     libsegengine's own sg_comm_* entry points (RCCL through the C ABI, include/segengine.h); the 128-byte
           RCCL id travels through the torch.distributed rendezvous store of whatever process group exists
           (gloo is enough), the collectives run on a HIP stream this module owns.
  "torch"  torch.distributed all_reduce on the default group (backend 'nccl' = RCCL on the GPU; 'gloo' on the CPU,
           which is what the world-size-2 tests here use).

xGMI is point-to-point (7 links/GPU): RCCL picks ring/tree per message size; buckets are kept large
(default 48 MB, ~6 for DeepLabv3+'s 258 MB) so each collective is bandwidth- rather than latency-bound.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple


def plan_buckets(param_ranges: List[Tuple[int, int, int]], total: int, bucket_elems: int) -> List[Tuple[int, int, int]]:
    """param_ranges: (node_index, offset, padded_size) of every trainable parameter in arena order.
    Returns buckets (start, end, ready_node_index) covering [0,total) exactly; a bucket is ready once the
    backward sweep (descending node index) has finished node `ready_node_index`."""
    buckets = []
    start, ready = 0, None
    for node_idx, off, size in param_ranges:
        if ready is None:
            ready = node_idx
        ready = min(ready, node_idx)
        end = off + size
        if end - start >= bucket_elems:
            buckets.append((start, end, ready))
            start, ready = end, None
    if start < total:
        buckets.append((start, total, ready if ready is not None else 0))
    return buckets


class TorchTransport:
    """torch.distributed collectives (nccl = RCCL on GPU tensors, gloo on CPU tensors)."""

    name = "torch"

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self._works = []

    def allreduce_async(self, t):
        self._works.append(self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))

    def join(self):
        for w in self._works:
            w.wait()  # stream-level dependency for nccl; blocks the host only for gloo
        self._works = []

    def broadcast(self, t, src=0):
        self.dist.broadcast(t, src=src, group=self.group)

    def barrier(self):
        self.dist.barrier(group=self.group)

    def scalar(self, v: float):
        """A one-element fp32 tensor where this transport can reduce it (device memory for nccl, host for gloo)."""
        import torch
        t = torch.tensor([float(v)], dtype=torch.float32)
        return t.cuda() if self.dist.get_backend(self.group) == "nccl" else t


def _unique_id(lib, _lib) -> bytes:
    """The 128 opaque bytes of an RCCL unique id (sg_comm_unique_id); raises SgError when RCCL cannot be loaded.  Rank 0
    only: ncclGetUniqueId starts a bootstrap root (listener thread + socket) that lives as long as the process."""
    buf = C.create_string_buffer(_lib.SG_COMM_ID_BYTES)
    _lib.check(lib.sg_comm_unique_id(buf), "sg_comm_unique_id")
    return bytes(buf.raw)


def _probe(lib, _lib) -> int:
    """Can THIS process load a usable RCCL (sg_comm_probe: dlopen + ncclGetVersion)?  Local, no bootstrap root, no socket -
    what every rank other than 0 calls (they used to draw and discard a unique id, leaking a listener thread
    and a port per rank, and could fail for network-interface reasons that have nothing to do with "library missing")."""
    v = C.c_int(0)
    _lib.check(lib.sg_comm_probe(C.byref(v)), "sg_comm_probe")
    return int(v.value)


class CommInitError(RuntimeError):
    """sg_comm_init (ncclCommInitRank) failed or timed out on at least one rank.  EVERY rank raises this after the same
    host-side exchange.  `stuck` is True on a rank whose own call never returned: its thread is still inside RCCL and
    cannot be cancelled, so the process must END (os._exit in bench.py) - never be re-used or re-exec'ed, it has touched
    the GPU - and the job be restarted as fresh processes."""

    def __init__(self, msg, stuck=False):
        super().__init__(msg)
        self.stuck = stuck


def _init_timeout_s() -> float:
    from . import switches
    return switches.get("SG_COMM_INIT_TIMEOUT")


def _comm_init(lib, _lib, uid, rank, world, device_index, timeout_s):
    """sg_comm_init on a worker thread, bounded by `timeout_s`.  -> (handle | None, error text | None, stuck).
    ncclCommInitRank is a collective with no timeout of its own: if ONE rank fails inside it (a fabric fault, a device it
    cannot open) the others wait for ever.  The call therefore runs on a daemon thread (ctypes drops the GIL; sg_comm_init
    sets the device itself, and a communicator may be used from another thread than the one that made it) while this
    thread waits with a deadline; sg_last_error() is thread-local, so the message is taken on the worker."""
    import threading
    box = {}

    def work():
        h = C.c_void_p()
        rc = lib.sg_comm_init(uid, rank, world, device_index, C.byref(h))
        msg = None
        if rc != 0:
            try:
                msg = lib.sg_last_error().decode("utf-8", "replace")
            except Exception:
                msg = "?"
        box.update(rc=rc, h=h, msg=msg)
    th = threading.Thread(target=work, name="sg_comm_init", daemon=True)
    th.start()
    th.join(timeout_s)
    if th.is_alive():
        return None, f"sg_comm_init did not return within {timeout_s:.0f} s (SG_COMM_INIT_TIMEOUT)", True
    if box["rc"] != 0:
        return None, f"sg_comm_init failed ({box['rc']}): {box['msg']}", False
    return box["h"], None, False


class SgTransport:
    """RCCL through libsegengine's C ABI (sg_comm_*), on a communication stream of its own.

    allreduce_async(t): the comm stream waits for everything queued so far on the compute stream (the kernels that
    produced `t`), then runs the in-place sum; join(): the compute stream waits for the comm stream.  No host sync."""

    name = "sg"

    def __init__(self, device, group=None):
        import torch
        import torch.distributed as dist
        from . import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.device = torch.device("cuda", device) if isinstance(device, int) else device
        # Step 1 - readiness.  EVERY rank probes its own RCCL first, locally (rank 0 by drawing the id: sg_comm_unique_id;
        # the others with sg_comm_probe = dlopen + ncclGetVersion, no bootstrap root; the one failure DataParallel's
        # "sg_or_torch" fallback exists for is "no usable librccl for dlopen"), then all ranks exchange (ok, message) AND
        # rank 0's id in ONE host-side collective.  Only when every rank is ready does anybody enter sg_comm_init
        # (ncclCommInitRank, itself a collective): a rank whose library is missing can never leave the others waiting inside
        # it, and all ranks raise the same error after the same collective.
        mine = [None, None]
        try:
            mine[0] = _unique_id(self.lib, _lib) if self.rank == 0 else (_probe(self.lib, _lib) >= 0)
        except Exception as e:
            mine[1] = f"{type(e).__name__}: {e}"
        everyone = [None] * self.world
        dist.all_gather_object(everyone, (mine[0] if self.rank == 0 else (mine[0] is not None), mine[1]), group=group)
        bad = [(r, m) for r, (ok, m) in enumerate(everyone) if not ok]
        if bad:
            raise _lib.SgError("RCCL is not usable (sg_comm_unique_id / sg_comm_probe) on rank(s) " + ", ".join(f"{r}: {m}" for r, m in bad))
        uid = everyone[0][0]
        # Step 2 - the communicator, with a deadline.  A failure INSIDE ncclCommInitRank on one rank used
        # to leave the others in that collective for ever.  Now every rank's call is bounded (_comm_init), the outcomes are
        # exchanged on the host, and if ANY rank failed or timed out, ALL raise CommInitError - a rank that failed at once
        # reaches the exchange first and waits there (the host group's own timeout bounds that) until the stuck ranks'
        # deadlines bring them along.  Nobody is left hanging; callers exit non-zero (bench.py) and the job restarts as
        # fresh processes.
        h, err, stuck = _comm_init(self.lib, _lib, uid, self.rank, self.world, self.device.index, _init_timeout_s())
        outcomes = [None] * self.world
        dist.all_gather_object(outcomes, err, group=group)
        failed = [(r, m) for r, m in enumerate(outcomes) if m is not None]
        if failed:
            if h is not None:
                try:
                    self.lib.sg_comm_destroy(h)
                except Exception:
                    pass
            raise CommInitError("RCCL communicator not established; every rank gives up together - " +
                                "; ".join(f"rank {r}: {m}" for r, m in failed), stuck=stuck)
        self.h = h
        self.stream = torch.cuda.Stream(self.device)
        self._pending = False

    def _dtype(self, t):
        torch = self.torch
        return {torch.float32: self._lib.SG_F32, torch.bfloat16: self._lib.SG_BF16, torch.int64: self._lib.SG_I64}[t.dtype]

    def allreduce_async(self, t):
        torch = self.torch
        assert t.is_cuda and t.is_contiguous()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._lib.check(self.lib.sg_comm_allreduce_sum(self.h, C.c_void_p(self.stream.cuda_stream), self._dtype(t),
                                                       C.c_void_p(t.data_ptr()), t.numel()), "sg_comm_allreduce_sum")
        t.record_stream(self.stream)
        self._pending = True

    def join(self):
        if self._pending:
            self.torch.cuda.current_stream(self.device).wait_stream(self.stream)
            self._pending = False

    def broadcast(self, t, src=0):
        """Rank `src`'s values to every rank, as a sum of (t on src, zeros elsewhere) - set-up time only."""
        if self.rank != src:
            t.zero_()
        self.allreduce_async(t)
        self.join()

    def barrier(self):
        one = self.torch.zeros(1, dtype=self.torch.float32, device=self.device)
        self.allreduce_async(one)
        self.join()
        self.torch.cuda.current_stream(self.device).synchronize()

    def scalar(self, v: float):
        return self.torch.tensor([float(v)], dtype=self.torch.float32, device=self.device)

    def close(self):
        if getattr(self, "h", None):
            self.torch.cuda.synchronize(self.device)
            self.lib.sg_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_transport(comm: str, device, group=None, fallback_backend: str = "nccl"):
    """The gradient transport of a DataParallel model.

    comm: "torch" | "sg" | "sg_or_torch" | "auto" (torch on an nccl group, sg otherwise).  "sg_or_torch" falls back to
    torch.distributed when libsegengine cannot bring RCCL up on ANY rank.  The decision is a collective: in
    SgTransport.__init__ every rank probes its own librccl and all ranks exchange the outcome before anybody calls
    ncclCommInitRank, so either all ranks construct the transport or all raise the same error; the summed flag below then
    only confirms that they take the same branch.  A failure or hang INSIDE ncclCommInitRank is not a fallback case: the call
    is bounded by SG_COMM_INIT_TIMEOUT on every rank, the outcomes are exchanged, and all ranks raise CommInitError together
    (the caller exits non-zero; a rank whose call never returned has `stuck` set and must end its process).  `fallback_backend` is "nccl" in
    production; the CPU tests pass "gloo"."""
    import torch
    import torch.distributed as dist
    if comm == "auto":
        comm = "torch" if dist.get_backend(group) == "nccl" else "sg"
    if comm == "torch":
        return TorchTransport(group)
    if comm not in ("sg", "sg_or_torch"):
        raise ValueError(f"comm={comm!r}")
    tp, err = None, None
    try:
        tp = SgTransport(device, group)
    except CommInitError:   # ncclCommInitRank failed / timed out somewhere: the fabric is in doubt and threads may be stuck
        raise               # inside RCCL - not a case for a fallback onto the same RCCL; every rank raises this together
    except Exception as e:  # e.g. no usable librccl for dlopen
        err = e
    if comm == "sg":
        if tp is None:
            raise err
        return tp
    flag = torch.tensor([0 if tp is not None else 1], dtype=torch.int32)
    if dist.get_backend(group) == "nccl":
        flag = flag.to(device)
    dist.all_reduce(flag, group=group)
    if int(flag.item()) > 0:  # somebody failed: all fall back to torch.distributed
        import sys
        print(f"[dist] sg_comm transport unavailable ({err!r}); falling back to torch.distributed {fallback_backend}",
              file=sys.stderr)
        if tp is not None:
            tp.close()
        g2 = group if dist.get_backend(group) == fallback_backend else dist.new_group(backend=fallback_backend)
        tp = TorchTransport(g2)
    return tp


class BucketReducer:
    """Bucketed sum-all-reduce of a flat arena, fired bucket by bucket from the backward sweep (device-agnostic: the
    tests drive it with CPU tensors over gloo)."""

    def __init__(self, arena, buckets, transport=None, group=None):
        self.arena = arena
        self.tp = transport if transport is not None else TorchTransport(group)
        # fire in the order the backward sweep completes them: highest ready index first
        self.buckets = sorted(buckets, key=lambda b: -b[2])
        self.next = 0
        self.fired: List[Tuple[int, int]] = []  # (node index at which it fired, bucket start): for the tests

    def reset(self):
        self.next = 0
        self.fired = []

    def node_done(self, node_index: int):
        """Called after each node's backward (descending index): launch every bucket that is now complete."""
        while self.next < len(self.buckets) and self.buckets[self.next][2] >= node_index:
            s, e, _ = self.buckets[self.next]
            self.tp.allreduce_async(self.arena[s:e])
            self.fired.append((node_index, s))
            self.next += 1

    def will_fire(self, node_index: int) -> bool:
        """Will node_done(node_index) launch an all-reduce?  (The runtime joins its side stream first.)"""
        return self.next < len(self.buckets) and self.buckets[self.next][2] >= node_index

    def finish(self):
        self.node_done(-1)
        self.tp.join()


class DataParallel:
    """Attach to a compiled Model: `DataParallel(model)`; the model's train_on_batch then all-reduces."""

    def __init__(self, model, bucket_mb: float = 48.0, group=None, comm: str = "auto"):
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError("init torch.distributed before DataParallel (backend 'nccl' = RCCL for comm='torch'; "
                               "'gloo' is enough as the rendezvous of comm='sg')")
        self.model = model
        self.group = group
        self.bucket_elems = int(bucket_mb * (1 << 20) / 4)
        model.dist = self
        rt = model._runtime()
        self.tp = make_transport(comm, rt.eng.device, group)
        self.world, self.rank = self.tp.world, self.tp.rank
        # identical replicas: broadcast rank-0 weights and BN statistics once
        self.tp.broadcast(rt.w_train, src=0)
        self.tp.broadcast(rt.w_frozen, src=0)
        rt.weights_changed()
        self.buckets = plan_buckets(param_ranges(model), rt.g_train.numel(), self.bucket_elems)
        self.reducer = BucketReducer(rt.g_train, self.buckets, self.tp)
        rt.on_node_done = self.reducer.node_done
        rt.node_done_fires = self.reducer.will_fire

    def allreduce_grads(self, rt) -> float:
        self.reducer.finish()
        self.reducer.reset()
        return 1.0 / self.world

    def reduce_step_scalars(self, loss, counts):
        """Loss -> mean over the ranks (every rank's loss is the mean over its own equally sized shard), confusion
        counts -> sums: the logs then describe the global batch on every rank."""
        self.tp.allreduce_async(loss)
        if counts is not None:
            self.tp.allreduce_async(counts)
        self.tp.join()
        self.model._runtime().eng.scale(loss, 1.0 / self.world)
        return loss, counts

    def sync_moving_stats(self, rt):
        """BatchNorm moving mean / variance averaged over the replicas (each has followed its own shards): called
        when a checkpoint is written, never inside the step."""
        self.tp.allreduce_async(rt.w_frozen)
        self.tp.join()
        rt.eng.scale(rt.w_frozen, 1.0 / self.world)

    def barrier(self):
        self.tp.barrier()

    def any_failed(self, failed: bool) -> bool:
        """Collective OR of a per-rank failure flag (also a barrier): lets every rank leave a collective section the same
        way when one of them - rank 0 writing a checkpoint - hit an error."""
        t = self.tp.scalar(1.0 if failed else 0.0)
        self.tp.allreduce_async(t)
        self.tp.join()
        return float(t.item()) > 0.0


def param_ranges(model) -> List[Tuple[int, int, int]]:
    """(node index, arena offset, padded size) of every trainable parameter, in arena (= creation) order."""
    return [(n.index, p.offset, (p.size + 3) // 4 * 4) for n in model.nodes for p in n.params if p.trainable]
