"""Worker of tests/test_hip_epochs.py::test_two_ranks_log_the_same_validation_values (2 ranks, gloo, both on cuda:0): every rank runs
SequenceTrainer.valid_epoch on its shard of the validation sequences (batches of 1, rank r takes r, r + world, ...); rank 0 also runs
the whole set in one process (no group) for comparison.  Prints one JSON line."""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]


class Shard(torch.utils.data.Sampler):
    def __init__(self, indices):
        self.indices = indices

    def __iter__(self):
        return iter(self.indices)

    def __len__(self):
        return len(self.indices)


def main():
    import epoch_recipe as E
    from util import build_hip_model, ref_cfg
    from rpg_ramnet_amd.parallel import shard_indices
    from rpg_ramnet_amd.trainer import SequenceTrainer
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    mcfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=E.K, loss_composition=["image", "events1"])
    model = build_hip_model("ERGB2DepthRecurrent", mcfg)            # torch.manual_seed(0): identical weights on every rank
    data = E.MemoryDataset(E.make_sequences(42, E.N_VALID, 0.05))
    train, _ = E.loaders()

    def loader(indices):
        return torch.utils.data.DataLoader(data, batch_size=1, sampler=Shard(indices))

    st = SequenceTrainer(E.CONFIG, model, train, loader(shard_indices(len(data), rank, world)), process_group=dist.group.WORLD)
    out = st.valid_epoch()
    if rank == 0:
        class Alone(SequenceTrainer):
            def _world(self):
                return 1
        out["single"] = Alone(E.CONFIG, model, train, loader(list(range(len(data))))).valid_epoch()
        assert Alone(E.CONFIG, model, train, loader(list(range(len(data))))).val_preview_indices == st.val_preview_indices
    print(json.dumps(out))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
