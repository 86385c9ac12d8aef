"""CPU, world_size 2, gloo: the Fourier view embedder's matrix under data parallelism.  Every rank draws its own B at construction;
`broadcast_parameters` replicates rank 0's once, beside the flat parameter buffer; the gradient all-reduce runs over the flat buffer, which
does not hold B: a step's gradient mean leaves it bit for bit what it was.  (tests/host_stub.HostStubNetwork: the real module wiring over a
closed-form CPU core, as in tests/test_dist_gloo.py.)"""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

B_KEY = "rendering_network.embedview_fn.B"


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _conf():
    from i2sdf_amd import plumbing_conf
    conf = plumbing_conf()
    r = conf["rendering_network"]
    del r["multires"]
    r.update(embed_type="fourier", channels=12, sigma=2.0)
    return conf


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from host_stub import HostStubNetwork
    from i2sdf_amd import dist as i2d
    torch.manual_seed(7 + rank)                      # every rank draws its own weights and its own B ...
    net = HostStubNetwork(_conf())
    net._ensure_flat()
    torch.manual_seed(7)
    ref = HostStubNetwork(_conf())
    ref._ensure_flat()
    own = net.state_dict()[B_KEY].clone()
    assert float(own.abs().max()) > 0 and (rank == 0) == torch.equal(own, ref.state_dict()[B_KEY])
    i2d.broadcast_parameters(net, src=0)             # ... until rank 0's are broadcast: the flat buffer, then the buffers
    assert torch.equal(net._flat, ref._flat) and torch.equal(net.state_dict()[B_KEY], ref.state_dict()[B_KEY])
    # B is no parameter: not in the flat buffer the gradient mean runs over, and a synchronised backward leaves it alone
    assert net._flat.numel() == sum(p.numel() for p in net.parameters()) and B_KEY not in dict(net.named_parameters())
    i2d.attach_data_parallel(net)
    seen = []
    sync = net.grad_sync
    net.grad_sync = lambda flat: (seen.append(flat.numel()), sync(flat))[1]
    g = torch.Generator().manual_seed(rank)
    out_ = net({"uv": torch.rand(16, 1, 2, generator=g) * 30})
    ((out_["rgb_values"] - torch.rand(16, 3, generator=g)) ** 2).mean().backward()
    assert seen == [net.layout.n_params]
    assert torch.equal(net.state_dict()[B_KEY], ref.state_dict()[B_KEY]) and net.rendering_network.embedview_fn.B.grad is None
    out.put((rank, True))
    dist.destroy_process_group()


def test_two_rank_gloo_replicates_the_fourier_matrix_and_never_reduces_it():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert sorted(q.get(timeout=5) for _ in range(2)) == [(0, True), (1, True)]
