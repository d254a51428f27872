"""The ten latent-update entries of the C ABI (Adam, SGD and Bop: flat, multi-tensor and fused with the
re-pack) refuse bad arguments exactly as they did before the flat and multi-tensor passes moved onto the
shared update policies: tests/golden/update_refusals.json holds (entry, case, return code, bnn_last_error())
of every case below, recorded from the library of the commit before that change.  Every case is refused by
an argument check, before any launch, so none of this needs a GPU; the pointers are never dereferenced.

    python tests/test_update_refusals.py        # re-record the golden file from the library in use
"""
import ctypes
import json
import math
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_refusals.json")
P = 4096                     # a 16-B aligned non-null address
NAN = math.nan

# the one text that changed on purpose: the device-step pack entry used to report the per-launch entry's name
RENAMED = {("bnn_adam_clamp_pack_sched", c): ("bnn_adam_clamp_pack:", "bnn_adam_clamp_pack_sched:")
           for c in ("p_null", "grad_null", "exp_avg_null", "exp_avg_sq_null", "N_zero", "K_zero", "N_negative",
                     "fmt_2", "nothing_to_write", "ldq_not_64", "ldq_short", "fp4_ldq_not_128", "ldqt_not_64",
                     "ldqt_short", "q_misaligned", "qt_fmt_3", "N_too_large")}

ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.0, clamp=1)
ADAM_SCHED = dict(beta1=0.9, beta2=0.999, eps=1e-8, sched=P, ctr=P, grad_scale=1.0, clamp=1)
SGD = dict(lr=0.1, momentum=0.9, omd=1.0, weight_decay=0.0, nesterov=0, first=0, grad_scale=1.0, clamp=1)
BOP = dict(gamma=1e-3, threshold=1e-6, grad_scale=1.0, flips=None)
PACK = dict(fmt=0, q=P, ldq=64, qt=None, ldqt=0, qt_fmt=0, stream=None)
ADAM_T = dict(p=P, grad=P, exp_avg=P, exp_avg_sq=P)
SGD_T = dict(p=P, grad=P, buf=P)
BOP_T = dict(w=P, grad=P, m=P)
# entry -> its arguments in the header's order, each with a value the entry accepts
BASE = {
    "bnn_adam_clamp": dict(**ADAM_T, n=8, **ADAM, stream=None),
    "bnn_adam_clamp_sched": dict(**ADAM_T, n=8, **ADAM_SCHED, stream=None),
    "bnn_adam_clamp_multi": dict(count=2, p=[P, P], grad=[P, P], exp_avg=[P, P], exp_avg_sq=[P, P], n=[8, 8],
                                 step=[1, 2], clamp=[1, 0], lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, sched=None,
                                 ctr=None, grad_scale=1.0, stream=None),
    "bnn_sgd_clamp": dict(**SGD_T, n=8, **SGD, stream=None),
    "bnn_sgd_clamp_multi": dict(count=2, p=[P, P], grad=[P, P], buf=[P, P], n=[8, 8], first=[0, 1], clamp=[1, 0],
                                lr=0.1, momentum=0.9, omd=1.0, weight_decay=0.0, nesterov=0, grad_scale=1.0,
                                stream=None),
    "bnn_bop": dict(**BOP_T, n=8, **BOP, stream=None),
    "bnn_adam_clamp_pack": dict(**ADAM_T, N=64, K=64, **ADAM, **PACK),
    "bnn_adam_clamp_pack_sched": dict(**ADAM_T, N=64, K=64, **ADAM_SCHED, **PACK),
    "bnn_sgd_clamp_pack": dict(**SGD_T, N=64, K=64, **SGD, **PACK),
    "bnn_bop_pack": dict(**BOP_T, N=64, K=64, **BOP, **PACK),
}
ARRAY_TYPES = {"n": ctypes.c_int64, "step": ctypes.c_int64, "clamp": ctypes.c_int32, "first": ctypes.c_int32}

SGD_HYPER = {"lr_negative": dict(lr=-0.1), "momentum_negative": dict(momentum=-0.5),
             "weight_decay_negative": dict(weight_decay=-1e-3), "omd_nan": dict(omd=NAN),
             "nesterov_without_momentum": dict(nesterov=1, momentum=0.0),
             "nesterov_with_dampening": dict(nesterov=1, omd=0.9)}
BOP_HYPER = {"gamma_zero": dict(gamma=0.0), "gamma_above_1": dict(gamma=1.5), "gamma_nan": dict(gamma=NAN),
             "threshold_negative": dict(threshold=-1.0), "threshold_nan": dict(threshold=NAN)}
PACK_CASES = {"N_zero": dict(N=0), "K_zero": dict(K=0), "N_negative": dict(N=-1), "fmt_2": dict(fmt=2),
              "nothing_to_write": dict(q=None, qt=None), "ldq_not_64": dict(K=100, ldq=100),
              "ldq_short": dict(K=100, ldq=64), "fp4_ldq_not_128": dict(fmt=1, K=256, ldq=64),
              "ldqt_not_64": dict(q=None, qt=P, ldqt=100), "ldqt_short": dict(N=100, q=None, qt=P, ldqt=64),
              "q_misaligned": dict(q=P + 4), "qt_fmt_3": dict(qt=P, ldqt=64, qt_fmt=3),
              "N_too_large": dict(N=64 * 65536)}


def _nulls(tensors):
    return {f"{t}_null": {t: None} for t in tensors}


def _second(field, value):
    """The multi-tensor arrays with tensor 1's ``field`` replaced."""
    return lambda base: {field: [base[field][0], value]}


MULTI_COUNT = {"count_17": dict(count=17), "count_negative": dict(count=-1)}
# entry -> {case: the arguments that differ from BASE (or a function of BASE giving them)}
CASES = {
    "bnn_adam_clamp": {**_nulls(ADAM_T), "n_negative": dict(n=-1), "step_0": dict(step=0),
                       "step_negative": dict(step=-3), "empty_step_0": dict(n=0, step=0)},
    "bnn_adam_clamp_sched": {**_nulls(ADAM_T), "n_negative": dict(n=-1), "sched_null": dict(sched=None),
                             "ctr_null": dict(ctr=None), "sched_and_ctr_null": dict(sched=None, ctr=None),
                             "empty_sched_null": dict(n=0, sched=None)},
    "bnn_adam_clamp_multi": {**MULTI_COUNT, **_nulls(("p", "grad", "exp_avg", "exp_avg_sq", "n", "step", "clamp")),
                             "lone_sched": dict(sched=P), "lone_ctr": dict(ctr=P),
                             "count_0_lone_sched": dict(count=0, sched=P),
                             "tensor_p_null": _second("p", None), "tensor_grad_null": _second("grad", None),
                             "tensor_exp_avg_null": _second("exp_avg", None),
                             "tensor_exp_avg_sq_null": _second("exp_avg_sq", None),
                             "tensor_n_negative": _second("n", -1), "tensor_step_0": _second("step", 0),
                             "empty_tensor_step_0": lambda b: dict(n=[8, 0], step=[1, 0])},
    "bnn_sgd_clamp": {**_nulls(SGD_T), "n_negative": dict(n=-1), **SGD_HYPER,
                      "empty_buf_null": dict(n=0, buf=None)},
    "bnn_sgd_clamp_multi": {**MULTI_COUNT, **_nulls(("p", "grad", "buf", "n", "first", "clamp")), **SGD_HYPER,
                            "tensor_p_null": _second("p", None), "tensor_grad_null": _second("grad", None),
                            "tensor_buf_null": _second("buf", None), "tensor_n_negative": _second("n", -1)},
    "bnn_bop": {**_nulls(BOP_T), "n_negative": dict(n=-1), **BOP_HYPER},
    "bnn_adam_clamp_pack": {**_nulls(ADAM_T), "step_0": dict(step=0), **PACK_CASES},
    "bnn_adam_clamp_pack_sched": {**_nulls(ADAM_T), "sched_null": dict(sched=None), "ctr_null": dict(ctr=None),
                                  **PACK_CASES},
    "bnn_sgd_clamp_pack": {**_nulls(SGD_T), **SGD_HYPER, **PACK_CASES},
    "bnn_bop_pack": {**_nulls(BOP_T), **BOP_HYPER, **PACK_CASES},
}


def _arg(name, v):
    if isinstance(v, list):                     # a host array of the multi-tensor entries
        ct = ARRAY_TYPES.get(name, ctypes.c_void_p)
        return ctypes.cast((ct * len(v))(*v), ctypes.c_void_p)
    return v


def refusals(lib):
    """[(entry, case, return code, error text)] of every case, in CASES' order."""
    out = []
    for entry, cases in CASES.items():
        for case, over in cases.items():
            args = dict(BASE[entry])
            args.update(over(args) if callable(over) else over)
            keep = [_arg(k, v) for k, v in args.items()]          # the arrays outlive the call
            rc = getattr(lib, entry)(*keep)
            out.append((entry, case, int(rc), lib.bnn_last_error().decode()))
    return out


@pytest.fixture(scope="module")
def lib():
    from bnn_amd import _lib
    return _lib.lib()


def test_update_entries_refuse_as_before(lib):
    with open(GOLDEN) as f:
        want = [tuple(r) for r in json.load(f)]
    got = refusals(lib)
    assert [r[:2] for r in got] == [r[:2] for r in want], "the case list and the golden file differ"
    assert len(want) > 150 and {r[0] for r in want} == set(BASE)
    for (entry, case, rc, text), (_, _, want_rc, want_text) in zip(got, want):
        assert want_rc != 0, (entry, case, "the golden file holds only refusals")
        if (entry, case) in RENAMED:
            old, new = RENAMED[(entry, case)]
            assert want_text.startswith(old)
            want_text = new + want_text[len(old):]
        assert (rc, text) == (want_rc, want_text), (entry, case)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "distributed-mnist-bnns_amd"))
    from bnn_amd import _lib
    with open(GOLDEN, "w") as f:
        json.dump(refusals(_lib.lib()), f, indent=0)
        f.write("\n")
