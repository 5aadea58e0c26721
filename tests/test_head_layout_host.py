"""The packed head-weight block: the UTTT_HEAD_* offsets of include/uttt_nn.h (what k_heads indexes) against
uttt_amd.nnfast._head_layout() (what pack_heads fills), and the element-to-index map the header states,
on a network whose every head parameter holds a value of its own. No GPU."""
import os
import re

import numpy as np

from conftest import REPO

NAMES = {"PCONV_W": "pconv_w", "PCONV_B": "pconv_b", "VCONV_W": "vconv_w", "VCONV_B": "vconv_b", "PFC_W": "pfc_w",
         "PFC_B": "pfc_b", "VFC1_W": "vfc1_w", "VFC1_B": "vfc1_b", "VFC2_W": "vfc2_w", "VFC2_B": "vfc2_b"}


def header_offsets():
    """The UTTT_HEAD_* #define chain evaluated in order: each body is integer arithmetic over earlier names."""
    text = open(os.path.join(REPO, "include", "uttt_nn.h")).read()
    env = {}
    for name, body in re.findall(r"^#define\s+(UTTT_HEAD_\w+)\s+(.+?)\s*$", text, re.M):
        assert re.fullmatch(r"[\w\s()+*]+", body), (name, body)
        env[name] = int(eval(body, {"__builtins__": {}}, dict(env)))  # noqa: S307 (the repository's own header)
    return env


def test_header_offsets_equal_the_python_layout():
    from uttt_amd.nnfast import _head_layout
    env, lay = header_offsets(), _head_layout()
    assert set(env) == {"UTTT_HEAD_" + k for k in NAMES} | {"UTTT_HEAD_SIZE"}
    for macro, key in NAMES.items():
        assert env["UTTT_HEAD_" + macro] == lay[key][0], (macro, env["UTTT_HEAD_" + macro], lay[key])
    assert env["UTTT_HEAD_SIZE"] == lay["size"]
    # the parts tile the block: each starts where the previous one ends
    spans = sorted(lay[k] for k in NAMES.values())
    assert spans[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] == lay["size"]


def distinct_head_network():
    """random_network(3) with an identity BatchNorm on both head convs except its bias (running mean 0,
    var 1 - eps, weight 1), so that fold_bn is exact, and every head parameter (the BN biases included) filled
    with consecutive integers: no two elements of the heads hold the same value."""
    import torch
    from uttt_amd.model import random_network
    net = random_network(3)
    base = 1
    with torch.no_grad():
        for bn in (net.policy_bn, net.value_bn):
            bn.running_mean.zero_()
            bn.running_var.fill_(1.0).sub_(bn.eps)
            bn.weight.fill_(1.0)
            assert torch.equal(bn.running_var + bn.eps, torch.ones_like(bn.running_var))  # the scale is exactly 1
        for t in (net.policy_conv.weight, net.policy_bn.bias, net.value_conv.weight, net.value_bn.bias,
                  net.policy_fc.weight, net.policy_fc.bias, net.value_fc1.weight, net.value_fc1.bias,
                  net.value_fc2.weight, net.value_fc2.bias):
            t.copy_(torch.arange(base, base + t.numel(), dtype=torch.float32).reshape(t.shape))
            base += t.numel()
    assert base - 1 < 2 ** 24  # every value an exact f32
    return net


def test_pack_heads_puts_every_element_where_the_header_says():
    import torch
    from uttt_amd.model import fold_bn
    from uttt_amd.nnfast import pack_heads
    env = header_offsets()
    net = distinct_head_network()
    for conv, bn in ((net.policy_conv, net.policy_bn), (net.value_conv, net.value_bn)):
        w, b = fold_bn(conv, bn)
        assert torch.equal(w, conv.weight) and torch.equal(b, bn.bias)  # the fold is exact here
    buf = pack_heads(net, "cpu").numpy()
    assert buf.dtype == np.float32 and buf.shape == (env["UTTT_HEAD_SIZE"],)
    assert len(np.unique(buf)) == buf.size  # every slot written once, from a different element
    at = lambda macro: env["UTTT_HEAD_" + macro]  # noqa: E731
    npy = lambda t: t.detach().numpy()  # noqa: E731
    pw, vw = npy(net.policy_conv.weight), npy(net.value_conv.weight)
    for p in range(2):
        for c in range(128):
            assert buf[at("PCONV_W") + p * 128 + c] == pw[p, c, 0, 0]
        assert buf[at("PCONV_B") + p] == npy(net.policy_bn.bias)[p]
    for c in range(128):
        assert buf[at("VCONV_W") + c] == vw[0, c, 0, 0]
    assert buf[at("VCONV_B")] == npy(net.value_bn.bias)[0]
    # policy FC, input-major: input j = plane * 81 + position (torch.flatten of NCHW), output o
    W = npy(net.policy_fc.weight)
    j, o = np.divmod(np.arange(162 * 81), 81)
    assert np.array_equal(buf[at("PFC_W") + j * 81 + o], W[o, j])
    assert np.array_equal(buf[at("PFC_B") + np.arange(81)], npy(net.policy_fc.bias))
    # value FC1, input-major: input j = position, unit u
    W1 = npy(net.value_fc1.weight)
    j, u = np.divmod(np.arange(81 * 256), 256)
    assert np.array_equal(buf[at("VFC1_W") + j * 256 + u], W1[u, j])
    assert np.array_equal(buf[at("VFC1_B") + np.arange(256)], npy(net.value_fc1.bias))
    assert np.array_equal(buf[at("VFC2_W") + np.arange(256)], npy(net.value_fc2.weight)[0])
    assert buf[at("VFC2_B")] == npy(net.value_fc2.bias)[0]
