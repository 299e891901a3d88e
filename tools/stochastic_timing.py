"""Step time of a stochastic NeuralNDCG job (BASELINE NeuralNDCG dimensions: bench.py's attn_neuralndcg model, 64 slates x 240,
stochastic=True, n_samples=32) through the autograd Trainer and through the fused, captured step.  usage (GPU box):
python tools/stochastic_timing.py ab      # both, in alternating windows of the same process; one JSON line
python tools/stochastic_timing.py fused   # 26 fused steps (for a kernel trace: tools/prof_summary.py <db> <title> <out.md> 26)"""
import json, os, sys, time
from functools import partial
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
from allrank_amd import _lib as LB, losses as E
from allrank_amd.engine import FusedTrainer, Trainer

w = bench.WORKLOADS["attn_neuralndcg"]
B, L, S = 64, 240, 32
args = dict(w["loss_args"], stochastic=True, n_samples=S)
dev = torch.device("cuda", 0)
x, y, idx = bench.synth_batch(4 * B, L, w["n_features"], 42, dev)
mode = sys.argv[1] if len(sys.argv) > 1 else "ab"


def stepper(tr):
    def step(i):
        j = (i % 4) * B
        return tr.step(x[j:j + B], y[j:j + B], idx[j:j + B])
    return step


def window(step, n):
    """the bench's step timing: a host clock around n steps that end in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


fused = stepper(FusedTrainer(bench.build_model(w, dev, 0.0), w["loss"], args, B, L, lr=1e-3, use_graph=True))
if mode == "fused":
    for i in range(26):
        fused(i)
    torch.cuda.synchronize()
    sys.exit(0)
m2 = bench.build_model(w, dev, 0.0)
auto = stepper(Trainer(m2, partial(getattr(E, w["loss"]), **args), torch.optim.Adam(m2.parameters(), lr=1e-3)))
for i in range(6):
    fused(i)
    auto(i)
rounds = {"fused_ms": [], "autograd_ms": []}
for r in range(5):                      # alternating windows: both see the same neighbours on the box
    rounds["fused_ms"].append(round(window(fused, 20), 4))
    rounds["autograd_ms"].append(round(window(auto, 20), 4))
med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
print(json.dumps({"slates": B, "slate_len": L, "n_samples": S, "steps_per_window": 20, "windows": rounds, "median": med,
                  "pseudo_slate_workspace_bytes": int(LB.lib().ltrx_neuralndcg_workspace_bytes(S * B, L, 50)),
                  "stream_arrays_bytes": 4 * S * B * L * 4}))
