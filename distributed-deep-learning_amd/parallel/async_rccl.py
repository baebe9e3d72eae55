"""Asynchronous parameter server over point-to-point RCCL, issued natively
(``csrc/kernels/rccl_async.hip``).

Reference (``mnist_async_sharding/worker.py:30-37,88-94``,
``parameter_server.py:94-111``): each worker Sends its gradient shards and blocks in Recv for
the parameters; each PS serves whichever push arrives (``ANY_SOURCE``), applies Adam with its
own step counter and Sends the parameters back.

Here every p2p transfer is part of an exclusive session between two processes (the kernel
file has the deadlock argument): one RCCL communicator, one comm stream and one native comm
thread per process; the initiating worker holds both processes' session locks (POSIX shm) and
posts ``(worker, ps)`` into the host's session mailbox.  This is the RCCL data plane of the
async modes; the xGMI one (``async_xgmi.py``) needs no p2p kernels and is the default on GPUs.
``self_sessions`` (W = 1) runs the exchange as send/recv to itself: the p2p path on one GPU.
"""
from __future__ import annotations

import contextlib
from typing import Dict

import torch
import torch.distributed as dist

from ..ops import native
from ..ops.adam import AdamHyper
from .comm import AsyncBase, DistEnv
from .ps import ParameterServer
from .sharding import ShardPlan


class RcclAsyncUnavailable(RuntimeError):
    pass


class RcclAsyncExchange(AsyncBase):
    backend = "rccl"
    unavailable = RcclAsyncUnavailable
    round_base = 1  # the service counts a worker's rounds at a PS from 1

    def __init__(self, plan: ShardPlan, env: DistEnv, params: torch.Tensor, grads: torch.Tensor,
                 servers: Dict[int, ParameterServer], steps_per_worker: int, job_id: str,
                 optimizer: str = "adam", check_provenance: bool = False, engine=None,
                 stage=None):
        if not params.is_cuda or not native.available():
            raise RcclAsyncUnavailable("needs the extension and a GPU")
        if env.world > 1 and env.backend != "nccl":
            raise RcclAsyncUnavailable("needs the nccl (RCCL) default group to exchange the id")
        if optimizer not in ("adam", "momentum", "sgd"):
            raise RcclAsyncUnavailable(f"no '{optimizer}' update")
        super().__init__(plan, env, params, grads, servers, steps_per_worker, check_provenance,
                         engine, stage)
        W, r = env.world, env.rank
        ps0 = next(iter(servers.values()), None)  # (a rank may host no PS)
        hyper = ps0.h if ps0 is not None else AdamHyper()
        mom = 0.0 if optimizer == "sgd" else (ps0.momentum if ps0 is not None else 0.9)
        wd, nesterov = (ps0.weight_decay, ps0.nesterov) if ps0 is not None else (0.0, False)
        ops = native.ops()
        ps_list = [(p, ps.params, ps.m, ps.v, ps.t) for p, ps in servers.items()]
        self.svc = ops.RcclAsync(params, grads, W, r, [tuple(map(int, x)) for x in self.ranges],
                                 [int(x) for x in self.hosts], ps_list,
                                 0 if optimizer == "adam" else 1, hyper.lr, hyper.beta1,
                                 hyper.beta2, hyper.eps, mom, W == 1, wd, nesterov)
        # communicator: rank 0's unique id over the default group (every rank joins)
        ids = [None]
        if r == 0:
            ids[0] = ops.SyncRunner.unique_id()
        if W > 1:
            dist.broadcast_object_list(ids, src=0)
        self.svc.init_comm(ids[0])
        # session locks (rank 0 creates the segment) and one session mailbox per rank
        if r == 0:
            self.svc.attach_shm(job_id, True)
        if W > 1:
            dist.barrier()
        if r != 0:
            self.svc.attach_shm(job_id, False)
        self.svc.open_boxes(True)
        if W > 1:
            dist.barrier()
        self.svc.open_boxes(False)

    def start(self) -> None:
        # the PS step counters may have been restored (checkpoint load) after the native object
        # copied them in __init__: hand the current ones over before the service runs
        for p, ps in self.servers.items():
            self.svc.set_t(p, int(ps.t))
        self.svc.start(self._expected(), self.check_provenance)

    def push_pull(self) -> None:
        self.svc.push_pull()

    @contextlib.contextmanager
    def paused(self):
        """Checkpoint hook: no session is served and no update issued inside the block."""
        self.svc.pause()
        try:
            self._sync_counters(self.svc.t)
            yield
        finally:
            self.svc.resume()

    def join(self) -> None:
        try:
            self.svc.join()
        finally:
            self._collect(self.svc.t, self.svc.served(), self.svc.provenance)
