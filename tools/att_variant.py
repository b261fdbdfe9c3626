"""Runs the config-3 step with attribute overrides (for rocprofv3): python tools/att_variant.py r_lstm=0.0"""
import sys
import torch
sys.path.insert(0, ".")
import bench
from switches import set_switches
dev = torch.device("cuda", 0)
model = bench.make_model("attention", dev, None)
for arg in sys.argv[1:]:
    k, v = arg.split("=")
    set_switches(model, {k: eval(v)})         # refuses a name the model's class does not declare
batch, _ = bench.synth(0, dev)
for _ in range(60):
    model.train_step(batch)
torch.cuda.synchronize()
