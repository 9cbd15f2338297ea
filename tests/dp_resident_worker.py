"""One data-parallel rank of tests/test_dp_resident_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_views_worker.py does).

DATA.device_resident under two ranks: train_net.build_loaders hands this rank its ResidentLoader over a label list of 12 entries (the two
bundled recordings, six times), global batch 4.  Two epochs are drawn; the parent gets every batch's recording indices, the fields the
loader delivered and the restatement of tests/resident_ref.py for the loader's own plan."""
import os
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
import resident_ref as rr                                                    # noqa: E402
from electrocardio_panorama_amd import train_net                             # noqa: E402
from electrocardio_panorama_amd.dataset import resident                      # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
work = pathlib.Path(out_dir) / f"rank{rank}"
work.mkdir(exist_ok=True)
cfg = rr.make_cfg(rr.write_listing(work, repeat=6), scheme=rr.SCHEMES[0])
cfg.DATA.device_resident = True
train, test = train_net.build_loaders(cfg, batch_size=4)
assert isinstance(train, resident.ResidentLoader) and (train.rank, train.world, train.batch_size) == (rank, 2, 2) and len(train) == 3
assert (test.rank, test.world, test.batch_size) == (0, 1, 4) and train.store.signal.is_cuda

FIELDS = ("data", "target_view", "rest_view", "rois", "input_theta", "target_theta", "rest_theta")
saved = {}
for epoch in range(2):
    train.sampler.set_epoch(epoch)
    idx, got, want = [], {k: [] for k in FIELDS}, {k: [] for k in FIELDS}
    for (_, batch, plan), meta in zip(train.plans(), train):
        idx.append(batch)
        ref = rr.plan_items(train.store, plan)
        for k in FIELDS:
            got[k].append(meta[k].cpu().numpy())
            want[k].append(ref[k])
    saved[f"idx{epoch}"] = np.array(idx)
    saved[f"order{epoch}"] = np.array(train.order())
    for k in FIELDS:
        saved[f"got{epoch}_{k}"], saved[f"want{epoch}_{k}"] = np.stack(got[k]), np.stack(want[k])
torch.cuda.synchronize()
dpc.save("resident", **saved)
dpc.finish("DPRESIDENT")
