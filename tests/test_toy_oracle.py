"""CPU check of tests/toy_oracle.py: a torch fp32/bf16 emulation of the toy
training step meets every bound the GPU tests
(test_toy_step_oracle_gpu.py) hold the kernels to, the integer-coded cases
pass their own exactness assertion and come out exact, and wrong steps are
SEEN: a 1 % gradient error by the f32 bound and by the zero-start bf16
case, a dropped row or column by the integer-coded cases even where the
bound cannot see it."""

import pytest
import torch

import toy_oracle as to
from toy_oracle import BF16, F32

# nine shapes from (1,1) to (128,20)
SHAPES = [(1, 1), (4, 4), (5, 3), (16, 16), (17, 17), (32, 20), (64, 20),
          (33, 32), (128, 20)]
SEEDS = range(20)
# storage, dy_bf16 (the wide-MFMA kernel's backward operand)
MODES = [(F32, False), (BF16, False), (BF16, True)]
MODE_IDS = ["f32", "bf16", "bf16-dybf16"]
# every power-of-two B the GPU file uses, at its K's
INT_SHAPES = [(1, 1), (4, 4), (16, 8), (16, 16), (32, 15), (32, 20),
              (64, 20), (64, 31), (16, 32), (128, 20), (64, 32), (128, 32)]


def _worst(kind, storage, dy_bf16, mutate=None, shapes=SHAPES):
    worst = to.Step(0.0, 0.0, 0.0, 0.0, 0.0)
    for B, K in shapes:
        for seed in SEEDS:
            x, t, w, b, lr = to.inputs(kind, B, K, storage, seed)
            ref, tol = to.toy_step_ref(x, t, w, b, lr, dy_bf16=dy_bf16,
                                       bf16_mfma=dy_bf16, storage=storage)
            got = to.emulate_step(x, t, w, b, lr, dy_bf16=dy_bf16,
                                  storage=storage, mutate=mutate)
            r = to.step_ratios(got, ref, tol, storage)
            worst = to.Step(*(max(a, c) for a, c in zip(worst, r)))
    return worst


@pytest.mark.parametrize("storage,dy_bf16", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", ["uniform", "signed", "normal100"])
def test_emulated_step_meets_every_bound(kind, storage, dy_bf16):
    worst = _worst(kind, storage, dy_bf16)
    print(f"{kind} {storage} dy_bf16={dy_bf16}: worst error/tol "
          + to.fmt_ratios(worst))
    assert max(worst) <= 1.0, to.fmt_ratios(worst)


@pytest.mark.parametrize("dy_bf16", [False, True], ids=["bf16", "bf16-dybf16"])
def test_zero_start_bf16_meets_bound_and_sees_one_percent(dy_bf16):
    worst = _worst("zero", BF16, dy_bf16)
    print(f"zero-start bf16 dy_bf16={dy_bf16}: worst error/tol "
          + to.fmt_ratios(worst))
    assert max(worst) <= 1.0, to.fmt_ratios(worst)
    # w' = -dw rounded once: a 1 % gradient error is 2.56 * 2^-8 of w'
    wrong = _worst("zero", BF16, dy_bf16, mutate="grad_1pct",
                   shapes=[(32, 20), (64, 20)])
    assert wrong.w > 1.0, to.fmt_ratios(wrong)


def test_f32_bound_sees_one_percent_and_bf16_params_at_small_lr_do_not():
    shapes = [(32, 20), (64, 20), (128, 20)]
    wrong = _worst("uniform", F32, False, mutate="grad_1pct", shapes=shapes)
    print("1 % gradient error, f32: error/tol " + to.fmt_ratios(wrong))
    assert wrong.w > 30 and wrong.dw > 30, to.fmt_ratios(wrong)
    # the reason for the integer-coded and zero-start cases: at lr 0.05 the
    # bf16 storage rounding hides the same error in a stored param of
    # ordinary size (lr * 1 % * |dw| against 2^-8 |w'|)
    x, t, w, b, lr = to.inputs("uniform", 32, 20, BF16, 0)
    ref, tol = to.toy_step_ref(x, t, w, b, lr, storage=BF16)
    big = ref.w.abs() > 0.25
    assert big.any()
    assert float((lr * 0.01 * ref.dw.abs() / tol.w)[big].max()) < 0.5


@pytest.mark.parametrize("mutate", ["no_bias", "half_scale"])
@pytest.mark.parametrize("storage,dy_bf16", MODES, ids=MODE_IDS)
def test_bound_sees_gross_errors(storage, dy_bf16, mutate):
    wrong = _worst("signed", storage, dy_bf16, mutate=mutate,
                   shapes=[(32, 20), (17, 17)])
    assert wrong.loss > 1.0 or wrong.dw > 1.0, to.fmt_ratios(wrong)


@pytest.mark.parametrize("storage,dy_bf16", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("B,K", INT_SHAPES)
def test_integer_coded_step_is_exact(B, K, storage, dy_bf16):
    x, t, w, b, lr = to.int_case(B, K, storage)
    # exact in the storage dtype
    for got, want in zip((x, t, w, b), to.int_case(B, K, torch.float64)[:4]):
        assert torch.equal(got.double(), want)
    ref = to.assert_step_exact(x, t, w, b, lr, dy_bf16=dy_bf16,
                               what=f"{B}x{K}")
    got = to.emulate_step(x, t, w, b, lr, dy_bf16=dy_bf16, storage=storage)
    for name in to.Step._fields:
        to.assert_equal_exact(getattr(got, name), getattr(ref, name),
                              f"{B}x{K} {name}")
    if B >= 16 and K >= 8:  # the step really moves the params
        assert float((ref.w - to.widen(w)).abs().max()) >= 0.25


@pytest.mark.parametrize("mutate", ["drop_row", "drop_col"])
@pytest.mark.parametrize("storage,dy_bf16", MODES, ids=MODE_IDS)
def test_integer_coded_step_sees_one_dropped_row_or_column(storage, dy_bf16,
                                                           mutate):
    for B, K in [(64, 20), (128, 32), (32, 15)]:
        x, t, w, b, lr = to.int_case(B, K, storage)
        ref = to.assert_step_exact(x, t, w, b, lr, dy_bf16=dy_bf16)
        got = to.emulate_step(x, t, w, b, lr, dy_bf16=dy_bf16,
                              storage=storage, mutate=mutate)
        with pytest.raises(AssertionError):
            for name in ("w", "b", "loss"):
                to.assert_equal_exact(getattr(got, name), getattr(ref, name))


def test_exactness_assertion_rejects_an_inexact_case():
    x, t, w, b, lr = to.int_case(32, 20)
    with pytest.raises(AssertionError):
        to.assert_step_exact(x, t, w * 0.3, b, lr)        # not integers
    with pytest.raises(AssertionError):
        to.assert_step_exact(x, t * 100, w, b, lr)        # |d| >= 256
    with pytest.raises(AssertionError):
        to.int_case(48, 20)                               # B not 2^n
