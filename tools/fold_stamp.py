"""Diagnostic: cycles per tile and wave of the folded last layer + heads (eg_gcn_layer_cls_fold_split_fwd), both roles, from a stamp
build of the library:  python echoglad_amd/build.py --variant=st -DEG_STAMP [-DEG_STAMP_PROD] [-DEG_FOLD_PROD_RB=R]
                       ECHOGLAD_LIB=echoglad_amd/lib/libechoglad_hip.st.so python tools/fold_stamp.py
The producers' four columns are descriptor wait + load issue, main stage, child sums + store, barrier + claim; with -DEG_STAMP_PROD
they are the wait at the first meeting, the residual product, the wait at the second meeting and the partial write instead
(FSPLIT, FOLD = 1).  The table of profiles/fold_handoff_ab.txt point 3 is one run of each build per R."""
import ctypes as ct
import os
import sys

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests", "golden"))
import torch  # noqa: E402

from echoglad_amd import _lib, ops  # noqa: E402
from echoglad_amd.nn._heads import fold_last_into_heads  # noqa: E402
from echoglad_amd.synthetic import synthetic_node_feats  # noqa: E402

DEV, B, WARM, LAUNCHES = "cuda:0", int(os.environ.get("EG_STAMP_B", "8")), 200, 20
g = ops.Graph.topo(224, 7)
x = synthetic_node_feats(B * g.num_nodes, 128, seed=1).to(DEV)
w = (synthetic_node_feats(128, 128, seed=2) * 0.1).to(DEV)
sc, sh = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
f = lambda *shape: (synthetic_node_feats(int(torch.tensor(shape).prod()), 1, 7).reshape(shape) * 0.1).to(DEV).contiguous()
packed = {"w1": f(128, 128), "s1": f(128) + 1, "t1": f(128), "w2": f(4, 16, 32), "s2": f(64) + 1, "t2": f(64), "w3": f(4, 16), "b3": f(4)}
fold = fold_last_into_heads(w, sc, sh, packed["w1"], packed["s1"], packed["t1"], True)
fold = fold + (ops.fold_lo_table(fold[0], fold[1]),)
ka = ops.new_kidsum(g, B)
h = ops.gcn_layer_fwd(g, B, x, w, sc, sh, x, relu=True, kidsum_out=ka)
lib = _lib.load()
buf = (ct.c_uint64 * 32)()
for _ in range(WARM):
    ops.gcn_layer_cls_fold_fwd(g, B, h, fold, True, packed, kidsum_in=ka)
lib.eg_debug_phase_cycles(g._h, buf, 1)
for _ in range(LAUNCHES):
    ops.gcn_layer_cls_fold_fwd(g, B, h, fold, True, packed, kidsum_in=ka)
lib.eg_debug_phase_cycles(g._h, buf, 1)
v = list(buf)
if not v[8]:
    sys.exit("no stamps: ECHOGLAD_LIB must name a library built with -DEG_STAMP")
tiles = g.num_tiles * B if hasattr(g, "num_tiles") else 1128 * B
per = lambda c: round(c / LAUNCHES / 4 / tiles)          # four waves per role
print("consumers  setup, tail, barrier, chain:             ", [per(c) for c in v[0:4]])
print("producers  (see the head of this file):            ", [per(c) for c in v[4:8]])
print(f"tile loop: {v[9] / LAUNCHES / tiles:.0f} cycles per tile and workgroup, clock {v[9] / max(v[10], 1) * 0.1:.3f} GHz")
