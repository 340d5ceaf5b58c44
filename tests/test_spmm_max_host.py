"""CPU checks of the max-aggregation training entries: argument errors without a GPU, a spill-free compile of spmm.hip
for gfx950, and the Citeseer-shaped synthetic graph of the example driver."""
import ctypes
import os
import re
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_max_entries_reject_bad_arguments_before_any_launch(hiplib):
    E, NULL = -1, None
    one = ctypes.c_int64(0)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)          # a non-NULL host pointer: never dereferenced on these paths
    f = hiplib.ocn_spmm_csr_max_arg
    assert f(p, p, NULL, -1, p, 64, p, p, NULL) == E                 # negative size
    assert f(p, p, NULL, 4, p, 48, p, p, NULL) == E                  # unsupported width
    assert f(p, p, NULL, 4, p, 1024, p, p, NULL) == E
    for i in (0, 1, 4, 6, 7):                                        # rowptr, col, x, y, arg
        args = [p, p, NULL, 4, p, 64, p, p, NULL]
        args[i] = NULL
        assert f(*args) == E, i
    b = hiplib.ocn_spmm_max_backward
    assert b(p, p, NULL, -1, p, p, 64, p, NULL) == E
    assert b(p, p, NULL, 4, p, p, 0, p, NULL) == E
    assert b(p, p, NULL, 4, p, p, 100, p, NULL) == E
    for i in (0, 1, 4, 5, 7):                                        # rowptrT, colT, arg, g, gx
        args = [p, p, NULL, 4, p, p, 64, p, NULL]
        args[i] = NULL
        assert b(*args) == E, i
    assert f(p, p, NULL, 0, p, 64, p, p, NULL) == 0                  # no rows: nothing to launch
    assert b(p, p, NULL, 0, p, p, 64, p, NULL) == 0


def test_spmm_kernels_do_not_spill(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "spmm.s"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"),
                    os.path.join(ROOT, "ocn_amd", "csrc", "spmm.hip"), "-o", str(out)], check=True, capture_output=True)
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", out.read_text(), re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", body)
        seen[kernel] = (spills, int(scratch.group(1)) if scratch else 0)
    assert sum("spmm_max_arg_kernel" in k for k in seen) == 6
    assert sum("spmm_max_backward_kernel" in k for k in seen) == 6
    assert all(v == (0, 0) for v in seen.values()), {k: v for k, v in seen.items() if v != (0, 0)}


def test_citeseer_shape_is_a_symmetric_graph_of_the_stated_size():
    from ocn_amd.synth import SHAPES, dataset_like, loaddataset_like
    s = SHAPES["citeseer"]
    assert (s["n"], s["nnz"], s["max_deg"], s["feat"]) == (3327, 9104, 99, 3703)
    ei, n, _ = dataset_like("citeseer", seed=0)
    assert n == 3327 and 2 * ei.shape[1] == 9104
    assert bool((ei[0] != ei[1]).all())                              # no self loops
    key = torch.minimum(ei[0], ei[1]) * n + torch.maximum(ei[0], ei[1])
    assert torch.unique(key).numel() == ei.shape[1]                  # each undirected edge once
    deg = torch.bincount(torch.cat([ei[0], ei[1]]), minlength=n)
    assert int(deg.max()) <= 99
    data, split = loaddataset_like("citeseer")
    r, c, _ = data.adj_t.coo()
    fwd = set(zip(r.tolist(), c.tolist()))
    assert fwd == set(zip(c.tolist(), r.tolist()))                   # the driver's adjacency is symmetric
    assert data.x.shape == (3327, 3703)
