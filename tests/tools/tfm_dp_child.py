"""One rank of the data-parallel rehearsal of tests/test_transformer_gpu.py::test_two_ranks_over_gloo_*: dp_child.py's 'traj'
mode for CNNTransformerNetwork.  Launched as a FRESH process per rank:

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/tools/tfm_dp_child.py <tfm_model golden> <out.npz> <p>

Both ranks share cuda:0, gradients travel through gloo.  Rank 0 holds the golden's weights, every other rank a random
initialisation and another dropout seed: HotPathTrainer.sync_replicas must make them identical before the first update.
3 SGD steps on the golden batch, rank r on its window shard -> losses, final parameters, the dropout seed buffer."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    gold_path, out_path, p = sys.argv[1], sys.argv[2], float(sys.argv[3])
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import deepards_amd.models as M
    from deepards_amd.train import HotPathTrainer, shard_windows
    from oracle.weights import seeded_params

    g = np.load(gold_path, allow_pickle=False)
    backbone = str(g['backbone'])
    torch.manual_seed(1234 + rank)                                   # different random init per rank
    bb = M.resnet18(first_pool_type=str(g['first_pool_type'])) if backbone == 'resnet18' else M.densenet18(drop_rate=0.0)
    model = M.CNNTransformerNetwork(bb, 0, False, int(g['hidden']), int(g['blocks']))
    if rank == 0:                                                    # only rank 0 holds the golden's weights
        sd = {k: torch.from_numpy(v) for k, v in seeded_params(backbone, int(g['seed']), bn_bias_shift=float(g['bn_bias_shift']),
                                                               head='single_breath').items() if k.startswith('breath_block.')}
        sd.update({k[len('param/'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('param/')})
        assert not model.load_state_dict(sd, strict=False).unexpected_keys
    for blk in model.transformer.blocks:
        blk.dropout = p
    model = model.cuda().train()
    model.transformer._drop_seed.fill_(1000 * rank)                  # rank 0's seed must replace it
    tr = HotPathTrainer(model, optimizer='sgd', world_size=world, rank=rank, use_graph=os.environ.get('DP_CHILD_GRAPH', '1') == '1')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    sl = shard_windows(x.shape[0], world, rank)
    out = {'losses': np.array([float(tr.train_step(x[sl].contiguous(), t[sl].contiguous())) for _ in range(3)])}
    torch.cuda.synchronize()
    for n, q in model.named_parameters():
        out['p/' + n] = q.detach().cpu().numpy()
    out['seed'] = model.transformer._drop_seed.cpu().numpy()
    out['allreduce_calls'] = np.array(tr.allreduce_calls)
    np.savez(out_path, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
