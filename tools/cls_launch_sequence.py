"""Every launch the classifier block's dispatch (csrc/classifier_kernels.hip) can make, once, in a fixed order: at the shapes
C1, C2, C4, B37, cls257 and simple of tests/test_gpu_classifier_train.py, both blocks, `phases` 1..63 and 123 with d_x given and
NULL (a refused combination returns before it launches and is skipped), one classifier_forward and one classifier_backward per
shape; the three BUCKET_SHAPES the same way through the *_bucketed entry points.  Eager, a few seconds.

Run it under a kernel trace with two builds of the library; the flat sequences of (kernel, grid, workgroup, LDS) must agree:
    rocprofv3 --kernel-trace --output-format csv -d OUT_A -- python tools/cls_launch_sequence.py --lib A/libnnue_hip.so
    rocprofv3 --kernel-trace --output-format csv -d OUT_B -- python tools/cls_launch_sequence.py
    python tools/cls_launch_sequence.py --compare OUT_A/.../*_kernel_trace.csv OUT_B/.../*_kernel_trace.csv
"""
import argparse
import csv
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "nnue-vision_amd"))

SHAPES = {  # B, L1, L2, L3, C
    "C1": (32, 64, 32, 8, 10),
    "C2": (512, 1024, 128, 32, 10),
    "C4": (128, 1024, 128, 32, 1000),
    "B37": (37, 256, 48, 16, 7),
    "cls257": (40, 320, 160, 40, 257),
    "simple": (33, 24, 7, 5, 3),
}
BUCKET_SHAPES = {"K3": (96, 256, 32, 16, 10, 3), "K8": (200, 1024, 128, 32, 100, 8), "K3simple": (37, 24, 8, 5, 3, 3)}
PHASES = tuple(range(1, 64)) + (123,)


def drive(lib_path):
    import torch
    from nnue_hip import lib as hip
    if lib_path:
        hip.LIB_PATH = Path(lib_path).resolve()
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(7)
    accepted = refused = 0
    for name, shape in {**SHAPES, **BUCKET_SHAPES}.items():
        B, L1, L2, L3, C = shape[:5]
        K = shape[5] if len(shape) > 5 else 1
        lead = (K,) if K > 1 else ()
        rnd = lambda *s: (torch.randn(*s, generator=gen) * 0.1).to(dev)  # noqa: E731
        x = torch.rand(B, L1, generator=gen).to(dev)
        w = (rnd(*lead, L2, L1), rnd(*lead, L2), rnd(*lead, L3, L2), rnd(*lead, L3), rnd(*lead, C, L3), rnd(*lead, C))
        labels = torch.randint(0, C, (B,), generator=gen).to(dev)
        plan = hip.bucket_group(torch.randint(0, K, (B,), generator=gen).to(dev, torch.int32), 0, K) if K > 1 else None
        scratch = torch.zeros(hip.classifier_train_scratch_bytes(B, L1, L2, L3, C, K), dtype=torch.uint8, device=dev)
        for pairwise in ((True,) if K > 1 else (True, False)):
            for phases in PHASES:
                for want_dx in (True, False):
                    try:
                        hip.classifier_train_step(x, pairwise, *w, labels, 1.0, 0.0, want_dx=want_dx, scratch=scratch, phases=phases,
                                                  buckets=plan)
                        accepted += 1
                    except hip.NnueHipError:
                        refused += 1
            h1, h2, logits = hip.classifier_forward(x, pairwise, *w, buckets=plan)
            hip.classifier_backward(x, pairwise, w[0], w[2], w[4], h1, h2, torch.softmax(logits, 1) / B, buckets=plan)
        torch.cuda.synchronize()
    print(f"train-step calls accepted {accepted}, refused {refused}")


def sequence(path):
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
             r["Workgroup_Size_Z"], r["LDS_Block_Size"]) for r in rows]


def compare(a, b):
    sa, sb = sequence(a), sequence(b)
    first = next((i for i, (p, q) in enumerate(zip(sa, sb)) if p != q), None)
    print(f"{len(sa)} and {len(sb)} kernels, {len(set(r[0] for r in sa))} distinct names")
    if first is not None or len(sa) != len(sb):
        i = first if first is not None else min(len(sa), len(sb))
        print(f"DIFFERENT from dispatch {i}: {sa[i:i + 1]} != {sb[i:i + 1]}")
        return 1
    print("launch sequences are equal")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build of libnnue_hip.so to drive")
    ap.add_argument("--compare", nargs=2, metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    drive(a.lib)
