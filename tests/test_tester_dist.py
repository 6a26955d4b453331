"""CPU, two gloo ranks: the tester's records are gathered as objects and merged by scene name on rank 0.  DistributedSampler pads
the last round with a repeated scene, so summing the ranks' counts would count it twice; the reference's dict.update keeps one."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _counts(seed):
    g = np.random.RandomState(seed)
    inter = g.randint(0, 50, 4)
    return dict(intersection=inter, union=inter + g.randint(1, 50, 4), target=inter + g.randint(0, 30, 4))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from scenesplat_amd.pointcept_api import engine, final_metrics, gather_records
    engine.init_distributed("gloo")
    # three scenes over two ranks: rank 0 gets scene0 + scene2, rank 1 gets scene1 + scene0 again (the sampler's padding)
    mine = {0: {"scene0": _counts(0), "scene2": _counts(2)}, 1: {"scene1": _counts(1), "scene0": _counts(0)}}[rank]
    merged = gather_records(mine)
    q.put((rank, None if merged is None else (sorted(merged), final_metrics(merged)["allAcc"])))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_records_of_two_ranks_are_merged_by_scene_on_rank_0():
    from scenesplat_amd.pointcept_api import final_metrics
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    res = dict(q.get(timeout=100) for _ in range(world))
    [p.join(30) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    assert res[1] is None
    names, all_acc = res[0]
    assert names == ["scene0", "scene1", "scene2"]
    assert all_acc == final_metrics({f"scene{i}": _counts(i) for i in range(3)})["allAcc"]
