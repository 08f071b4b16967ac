#!/usr/bin/env python3
"""Neighbour-sampled training (an addition; the reference trains full-batch only): draw one mini-batch with
NeighborSampler and look at it, then let experiment() train GraphSAGE on batches of 256 seeds with fan-outs [10, 5].
Needs an MI355X: the sampler draws with HIP kernels and has no CPU fallback.

    python examples/neighbor_sampling_example.py [model_name]        # graphsage | graphsage2 | gat | gin | ...
"""
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgb_experiment_amd import InitialParameters, NeighborSampler, experiment  # noqa: E402
from simple_example import write_cora_shaped  # noqa: E402

if __name__ == "__main__":
    model_name = sys.argv[1] if len(sys.argv) > 1 else "graphsage"
    dev = torch.device("cuda:0")
    n = 5000
    edge_index = torch.randint(0, n, (2, 60000), generator=torch.Generator().manual_seed(0)).to(dev)
    sampler = NeighborSampler(edge_index, n, num_neighbors=[10, 5])
    batch = sampler.sample(torch.arange(0, 64, device=dev), seed=(1, 2))
    print(f"64 seeds -> {batch.n_id.numel()} nodes, {batch.e_id.numel()} edges; the first edges in global ids:")
    print(torch.stack([batch.n_id[batch.edge_index[0, :5]], batch.n_id[batch.edge_index[1, :5]]]).tolist(),
          "=", edge_index[:, batch.e_id[:5]].tolist())
    with tempfile.TemporaryDirectory() as root:
        dataset_name = write_cora_shaped(root)
        acc_dict = experiment(model_init_param=InitialParameters.defaults_for(model_name), dataset_name=dataset_name,
                              dataset_root=root, dataset_split_mode="ratio", model_name=model_name,
                              dataset_split_seed=14530529, learning_rate=0.01, epoch=20, normalize_feature="row",
                              num_neighbors=[10, 5], batch_size=256)
    print(acc_dict)
