"""What does v_mfma_f32_32x32x16_fp8_fp8 keep of a small product beside a large one?  Read through the fp8 attention forward's stored P
(ops.attention_fwd(fp8=True, want_p=True)): every key shares one large product 448 * q0 with the query, key j adds one small product, and
log(P_ij / P_i0) / scale is what the score kept of it.  Printed per q0: the small product in the large one's group of 8 channels, in another
K-step, and two keys whose extra is spread over many products.  Result on an MI355X (tests/attn_ref.py, Quantities): the 8 products a lane
supplies are aligned to the largest exponent sum e among them and lose what lies below 2^(e - 13); across groups the sum is fp32.
    python tools/fp8_mfma_probe.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from generative_models_amd import ops

C, N = 128, 64
scale = C ** -0.5
big = [0, 1, 4, 16, 32, 64, 128, 256, 384, 448]
small = [2.0 ** e for e in range(-3, 7)]
qkv = torch.zeros((1, N, 3 * C))
q, k = qkv[0, :, :C], qkv[0, :, C:2 * C]
for i in range(N):
    q[i, 0] = big[i % len(big)]
    q[i, 1] = 1
    q[i, 17] = 1
    if i >= 30:                 # these queries carry 14 more unit products in the big product's K-step and 100 elsewhere
        q[i, 2:16] = 1
        q[i, 28:128] = 1
k[:, 0] = 448
for n, s in enumerate(small):
    k[1 + n, 1] = s
    k[11 + n, 17] = s
k[:, 2:16] = 0.5                # only seen by queries >= 30; the same for every key: cancels exactly if nothing is lost
k[:, 28:128] = 0.5
k[21, 2:16] = 1.0               # key 21: +7 in the same K-step, spread over 14 products of 0.5 extra
k[22, 28:128] = 0.625           # key 22: +12.5 spread over 100 products of 0.125 extra in the other K-steps
o, P = ops.attention_fwd(qkv.bfloat16().cuda(), scale, want_p=True, fp8=True)
P = P[0].double().cpu()
d = torch.log(P / P[:, :1]) / scale
torch.set_printoptions(linewidth=250, precision=3, sci_mode=False)
print("rows: big product 448 * q0; columns: small product in the same K-step (exact value on top)")
print("exact   ", small)
for i in list(range(10)) + list(range(30, 40)):
    print(f"q0={float(q[i, 0]):5.0f} {'+fill' if i >= 30 else '     '} same K-step ", [round(float(x), 3) for x in d[i, 1:11]])
    print(f"                 other K-step", [round(float(x), 3) for x in d[i, 11:21]], " key21 (+7):", round(float(d[i, 21]), 3), " key22 (+12.5):", round(float(d[i, 22]), 3))
