"""The fp32 multi-step kernel selector (chain | mfma): process-wide state in
the native extension, initialised from MI355X_TOY_MULTISTEP. Host-side
only — no kernel is launched here."""

import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ext():
    from mi355x_ddp import ops
    return ops.ext()


def test_set_get_roundtrip_and_rejects_unknown_names():
    ext = _ext()
    before = ext.get_toy_multistep_impl()
    try:
        for name in ("mfma", "chain"):
            ext.set_toy_multistep_impl(name)
            assert ext.get_toy_multistep_impl() == name
        with pytest.raises(RuntimeError):
            ext.set_toy_multistep_impl("valu")
        assert ext.get_toy_multistep_impl() == "chain"  # unchanged by the error
        for depth in (0, 2, 3, 4):
            ext.set_toy_multistep_chain_depth(depth)
        for depth in (1, 5, -1):
            with pytest.raises(RuntimeError):
                ext.set_toy_multistep_chain_depth(depth)
    finally:
        ext.set_toy_multistep_impl(before)
        ext.set_toy_multistep_chain_depth(0)


@pytest.mark.parametrize("value,expect", [(None, "chain"), ("chain", "chain"),
                                          ("mfma", "mfma")])
def test_env_knob_initialises_the_selector(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "MI355X_TOY_MULTISTEP"}
    if value is not None:
        env["MI355X_TOY_MULTISTEP"] = value
    code = ("import sys; sys.path.insert(0, %r); from mi355x_ddp import ops; "
            "print(ops.ext().get_toy_multistep_impl())" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    assert out.stdout.strip().splitlines()[-1] == expect
