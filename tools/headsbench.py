"""Time ocn_heads_fused alone:
    python tools/headsbench.py
All rows run all branches (no class ranges): 8 panels per 128-row tile."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ocn_amd.model as M  # noqa: E402

dev = torch.device("cuda:0")
for H, B in ((256, 65536), (128, 32768)):
    torch.manual_seed(0)
    pred = M.predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(dev).eval()
    x1, x2, xij = (torch.randn(B, H, device=dev) for _ in range(3))
    with torch.no_grad():
        for _ in range(5):
            pred._heads_fused(x1, x2, xij, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = int(os.environ.get("HB_N", 20))
        for _ in range(n):
            pred._heads_fused(x1, x2, xij, None)
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    fl = 2.0 * H * H * 8 * B
    print(f"H={H} B={B}: {dt * 1e6:8.1f} us  {fl / dt / 1e12:6.1f} TF f32-equivalent  {6 * fl / dt / 1e15:5.2f} PF bf16 issued", flush=True)
