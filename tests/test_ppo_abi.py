"""libnmmo_ppo.so (include/nmmo_ppo.h) loads without a GPU, its ctypes mirror matches the header,
and it reports argument errors through the return code + nmp_last_error without touching a GPU.
Its exports and source hash: tests/test_native_libs.py. CPU only."""

import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nmmo_ppo.h")
P = 0x1000  # a non-null dummy pointer: never dereferenced


@pytest.fixture(scope="module")
def ppo():
    from nmmo_amd import ppo

    ppo.lib()
    return ppo


def test_struct_and_constants_match_header(ppo):
    text = open(HEADER).read()
    for macro, val in [("NMP_OK", ppo.NMP_OK), ("NMP_E_INVALID", ppo.NMP_E_INVALID), ("NMP_E_HIP", ppo.NMP_E_HIP),
                       ("NMP_MAX_N", ppo.MAX_N), ("NMP_LOSS", ppo.LOSS), ("NMP_PG_LOSS", ppo.PG_LOSS),
                       ("NMP_V_LOSS", ppo.V_LOSS), ("NMP_ENTROPY", ppo.ENTROPY),
                       ("NMP_OLD_APPROX_KL", ppo.OLD_APPROX_KL), ("NMP_APPROX_KL", ppo.APPROX_KL),
                       ("NMP_CLIPFRAC", ppo.CLIPFRAC), ("NMP_N_STATS", ppo.N_STATS), ("NMP_ADV_MEAN", ppo.ADV_MEAN),
                       ("NMP_ADV_STD", ppo.ADV_STD), ("NMP_N_OUT", ppo.N_OUT)]:
        m = re.search(rf"#define {macro} (.*?)(?:/\*|$)", text, re.M)
        assert eval(m.group(1).strip()) == val, macro
    assert ctypes.sizeof(ppo.NmpParams) == 4 * 8 + 2 * 4
    fields = re.search(r"typedef struct NmpParams \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"(?:double|int32_t)\s+(\w+);", fields) == [f[0] for f in ppo.NmpParams._fields_]


def _loss(ppo, params="good", n=1024, ins=(P,) * 7, outs=(P,) * 5, accum=None):
    if params == "good":
        params = ppo.params_struct(0.1, 0.1, 0.01, 0.5)
    return ppo.lib().nmp_loss(None if params is None else ctypes.byref(params), n, *ins, *outs, accum, None)


def test_argument_errors_are_reported_without_a_gpu(ppo):
    """Every pointer is a non-null dummy that is never dereferenced: each call must fail its
    argument check before any launch."""
    L, E = ppo.lib(), ppo.NMP_E_INVALID

    def bad(what, **kw):
        assert _loss(ppo, **kw) == E, what
        assert what.encode() in L.nmp_last_error(), (what, L.nmp_last_error())

    bad("params is NULL", params=None)
    for i, name in enumerate(("clip_coef", "vf_clip_coef", "ent_coef", "vf_coef")):
        for v in (-0.1, -math.inf, math.inf, math.nan):
            coefs = [0.1, 0.1, 0.01, 0.5]
            coefs[i] = v
            bad(name, params=ppo.params_struct(*coefs))
    bad("n -1", n=-1)
    bad("n 16777217", n=ppo.MAX_N + 1)
    bad("norm_adv", n=1)
    for i in range(7):
        ins = [P] * 7
        ins[i] = None
        bad("input pointer is NULL", ins=tuple(ins))
    for i in range(5):
        outs = [P] * 5
        outs[i] = None
        bad("output pointer is NULL", outs=tuple(outs))
    # zero rows is a successful no-op that launches nothing, with or without an accumulator
    assert _loss(ppo, n=0) == ppo.NMP_OK
    assert _loss(ppo, n=0, accum=P) == ppo.NMP_OK
    # a NULL pointer is an error even then, and the extreme legal n passes the range check
    assert _loss(ppo, n=0, outs=(None,) + (P,) * 4) == E
    assert _loss(ppo, n=ppo.MAX_N, ins=(None,) + (P,) * 6) == E and b"NULL" in L.nmp_last_error()


def test_python_wrapper_rejects_host_tensors_and_bad_shapes(ppo):
    import torch

    x = torch.zeros(4)
    kw = dict(clip_coef=0.1, vf_clip_coef=0.1, ent_coef=0.01, vf_coef=0.5)
    with pytest.raises(ppo.PpoError):  # no torch fallback: host tensors are an error
        ppo.ppo_loss(x, x, x, x, x, x, x, **kw)


def test_train_config_switch_defaults_off():
    from nmmo_amd.trainer import TrainConfig

    assert TrainConfig().fused_loss is False
