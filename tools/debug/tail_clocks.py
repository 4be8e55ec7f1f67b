"""Phase clocks of tail_dx_train_kernel at a BASELINE workload (library built with NNUE_BUILD_ABLATIONS=1): the step runs
eagerly with NNUE_CLS_ABL_TAIL_CLOCKS=1, thread 0 of every workgroup leaves one shader-clock reading per phase boundary, and
this prints the mean / median cycles per phase over the workgroups of the last launch.
    NNUE_CLS_ABL_TAIL_CLOCKS=1 python tools/debug/tail_clocks.py [c2] [steps]"""
import ctypes, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nnue-vision_amd"))
sys.path.insert(0, ROOT)
os.environ.setdefault("NNUE_CLS_ABL_TAIL_CLOCKS", "1")
import nnue
from bench import OPT, WORKLOADS
from nnue_hip import lib as nlib
from nnue_hip.trainer import NnueTrainer

PHASES = ["entry loads + slab sum + h1", "h2 K quarters (MFMA)", "h2 sum + act", "logits (MFMA)", "softmax / CE", "d_z2 halves (MFMA)",
          "d_z2 sum + gate", "d_z1 (MFMA)", "d_x"]
NCLK = len(PHASES) + 1  # kTdxClocks of csrc/classifier_kernels.hip
which = sys.argv[1] if len(sys.argv) > 1 else "c2"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 12
cfg = WORKLOADS[which]
torch.manual_seed(0)
model = nnue.NNUE(nnue.GridFeatureSet(cfg["grid"], cfg["fps"]), cfg["l1"], cfg["l2"], cfg["l3"], num_classes=cfg["classes"],
                  input_size=cfg["image"], num_ls_buckets=cfg.get("buckets", 1), clip_activations=cfg.get("clip")).cuda()
tr = NnueTrainer(model, cfg["batch"], (cfg["image"], cfg["image"]), use_graph=False, input_slots=2, **OPT)
gen = torch.Generator().manual_seed(1234)
for im, lb in tr.inputs:
    im.copy_(torch.randn(cfg["batch"], 3, cfg["image"], cfg["image"], generator=gen))
    lb.copy_(torch.randint(0, cfg["classes"], (cfg["batch"],), generator=gen))
for _ in range(steps):
    tr.step()
torch.cuda.synchronize()
dll = ctypes.CDLL(str(nlib.LIB_PATH))
fn = dll.nnue_cls_abl_tail_clocks  # AttributeError: the library was not built with NNUE_BUILD_ABLATIONS=1
fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
buf = np.zeros((4096, NCLK), dtype=np.int64)
n = fn(buf.ctypes.data, buf.shape[0])
if n <= 0:
    sys.exit("no clocks: set NNUE_CLS_ABL_TAIL_CLOCKS=1 and run a shape the fused tail takes")
c = buf[:n]
c = c[c[:, 0] != 0]  # workgroups past the last row tile leave nothing
d = np.diff(c, axis=1)
print(f"{which}: {len(c)} workgroups, skip products = {os.environ.get('NNUE_CLS_ABL_SKIP_TAIL_PRODUCTS', '0')}")
for i, name in enumerate(PHASES):
    print(f"  {name:30s} mean {d[:, i].mean():8.0f}  median {np.median(d[:, i]):8.0f}  min {d[:, i].min():6d}  max {d[:, i].max():6d} cycles")
tot = c[:, -1] - c[:, 0]
print(f"  {'whole workgroup':30s} mean {tot.mean():8.0f}  median {np.median(tot):8.0f}  min {tot.min():6d}  max {tot.max():6d} cycles")
