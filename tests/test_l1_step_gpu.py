"""GPU: the fused d = 384 L1 step -- forward, backward (uniform and balanced row partition) and the gradient reduction -- element by
element against the float64 reference and the derived bounds of tests/l1_step_reference.py (where each term comes from: that module's
docstring; what the bounds catch: tests/test_l1_step_bound_cpu.py).

One engine run per case, shared by the tests through a module fixture.  Every case has d_p = 384:

    uniform           d 384, n 3072, M 1000 bf16     ragged M, copied x, uniform row ranges
    alias             n 1024, M 2048 bf16            aliased x (M = M_p), 64 steps on an engine whose cost model keeps the uniform form
    pad_d             d 380, n 200, M 1500 fp16      padded d and n, the forward's PAD instantiation
    fp32_x            n 3072, M 1024 fp32            the residual against the fp32 input
    bal_m3            n 3072, max_rows 31 744, M 2100 bf16   balanced, m = 3: straddling workgroups, 68 steps (q = 3: a clamped quantum, empty quanta)
    bal_m5            n 5000, max_rows 25 600, M 3000 fp32   balanced, m = 5, n no multiple of 128, 96 steps (no clamp)
    bal_m12           n 12 288, max_rows 4096, M 2048 bf16   balanced, m = 12, 3 - 4 pieces per tile, aliased x
    bal_as_uniform    bal_m3's batch, debug_flags 83          the same batch through the uniform form
    bal_scal          bal_m3's batch, debug_flags 78          alpha / count from the finalised scalars instead of the forward's counts
    second_step_700, second_step_2048   the bal_m3 engine, after its 2100-row batch: uniform (24 steps), then balanced again
                                        (64 steps, q = 2): slab pieces and pad rows that an earlier batch left
    after_update      the uniform engine after two optimizer updates: Wt as the folded update wrote it (the planted latents keep their
                      row sets; the activations are no longer exactly 7, the hot latent's zero column has become a unit vector)

The plan the engine reports (SaeEngine.l1_backward_plan) must equal the hard-coded one of the case: a precondition that fails, never
skips.  pytest -s prints the worst |difference| / tol per tensor and case."""
import numpy as np
import pytest

from tests import l1_step_reference as R
from tests.decode_reference import bf16, bits

pytestmark = pytest.mark.gpu

LR = 4e-4
CASE_NAMES = tuple(R.CASES)


def _engine(name):
    from freud_amd.engine import SaeEngine
    d, n, max_rows, _, _, flags, _, _ = R.CASES[name]
    return SaeEngine(variant="l1", d_model=d, n_dict=n, max_rows=max_rows, optimizer="adam", recon_alpha=R.ALPHA, debug_flags=flags)


def _batch(eng, case, load=True):
    """One forward_backward of the case's batch -> everything the tests look at, as host arrays."""
    d, n, M = case["d"], case["n"], case["M"]
    out = {"plan": eng.l1_backward_plan(M)}
    if load:
        eng.set_params({"decoder.weight": case["W"].numpy(), "encoder_bias": case["b"].numpy()})
    eng.forward_backward(case["x"].cuda())
    out["metrics"] = eng.metrics().copy()
    out["c"] = eng.debug_read(0, M * n).reshape(M, n)
    out["g"] = eng.debug_read(1, M * d).reshape(M, d)
    out["wt"] = eng.debug_read(15, n * d).reshape(n, d)
    grads = eng.debug_read(2, d * n + n)
    out["dW"], out["db"] = grads[:d * n].reshape(d, n), grads[d * n:]
    out["params"] = eng.get_params()
    return out


def _norm_check(eng, out):
    """optimizer_step's clip norm (metrics[3]) against the float64 norm of the gradient that was read back."""
    eng.optimizer_step(LR)
    want = float(np.sqrt((out["dW"].astype(np.float64) ** 2).sum() + (out["db"].astype(np.float64) ** 2).sum()))
    out["gnorm"] = (float(eng.metrics()[3]), want)


class Runs:
    """Lazy, cached engine runs: a case is executed when the first test asks for it (together with the cases that share its engine).
    Once an engine call has raised, no later test starts another run on the device: they fail with the first error."""

    def __init__(self):
        self.out, self.cases, self.broken = {}, {}, None

    def case(self, name):
        name = R.INPUTS_OF.get(name, name)
        if name not in self.cases:
            self.cases[name] = R.case_of(name)
        return self.cases[name]

    def get(self, name):
        if name not in self.out:
            assert self.broken is None, f"an earlier engine run failed: {self.broken}"
            group = {"second_step_700": "bal_m3", "second_step_2048": "bal_m3", "after_update": "uniform"}.get(name, name)
            try:
                getattr(self, "_run_" + ("bal_m3" if group == "bal_m3" else "uniform" if group == "uniform" else "single"))(group)
            except Exception as e:
                self.broken = repr(e)
                raise
        return self.out[name]

    def _twin(self, name):
        """A second engine on the same inputs: the gradient and the master it leaves."""
        eng = _engine(name)
        out = _batch(eng, self.case(name))
        eng.close()
        return out["dW"], out["db"], out["params"]

    def _run_single(self, name):
        eng = _engine(name)
        out = self.out[name] = _batch(eng, self.case(name))
        out["twin"] = self._twin(name)
        _norm_check(eng, out)
        eng.close()

    def _run_bal_m3(self, name):
        eng = _engine(name)
        for key in ("bal_m3", "second_step_700", "second_step_2048"):
            self.out[key] = _batch(eng, self.case(key))
        _norm_check(eng, self.out["second_step_2048"])
        eng.close()
        self.out["bal_m3"]["twin"] = self._twin("bal_m3")

    def _run_uniform(self, name):
        eng = _engine(name)
        case = self.case("uniform")
        out = self.out["uniform"] = _batch(eng, case)
        _norm_check(eng, out)                      # the first update
        eng.step(case["x"].cuda(), LR)             # the second
        self.out["after_update"] = _batch(eng, case, load=False)
        _norm_check(eng, self.out["after_update"])
        eng.close()
        out["twin"] = self._twin("uniform")

    def ops(self, name):
        out, case = self.get(name), self.case(name)
        if "ops" not in out:
            out["ops"] = R.operands(case["x"], out["wt"], out["params"]["encoder_bias"], out["c"], out["g"], case["alpha"])
        return out["ops"]

    def sums(self, name):
        """The plan-independent sums of the backward reference; bal_as_uniform and bal_scal read bal_m3's once their operands have been
        shown to be bitwise the same."""
        out = self.get(name)
        if "sums" not in out:
            base = self.out.get("bal_m3") if name in ("bal_as_uniform", "bal_scal") else None
            same = base is not None and "sums" in base and all(np.array_equal(bits(out[k]), bits(base[k])) for k in ("c", "g", "wt"))
            out["sums"] = base["sums"] if same else R.backward_sums(self.ops(name))
        return out["sums"]


@pytest.fixture(scope="module")
def runs():
    r = Runs()
    yield r
    r.out.clear()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_is_the_expected_form(runs, name):
    """The form that ran is asserted, not assumed: form, splits, m, q, grid, steps and tiles."""
    want = R.CASES[name][7]
    got = runs.get(name)["plan"]
    assert got == want, f"{name}: the engine plans {got}, the case was built for {want}"
    assert got["form"] == R.DW_FUSED and bool(got["balanced"]) == name.startswith(("bal_m", "bal_scal", "second_step_2048"))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_operands_and_exact_facts(runs, name):
    out, case = runs.get(name), runs.case(name)
    d, n, M = case["d"], case["n"], case["M"]
    R.assert_coverage(case, out["c"], exact=name != "after_update")
    # Wt is bf16 of the normalised master, to the bit
    assert np.array_equal(bits(out["wt"]), bits(bf16(out["params"]["decoder.weight"].T))), "Wt is not bf16(master^T)"
    assert out["metrics"][4] == float(M * d - case["masked"]), f"count {out['metrics'][4]}, wanted {M * d - case['masked']}"
    assert (out["c"] >= 0).all() and not np.signbit(out["c"]).any()
    keep = R.as_f32(case["x"]) != -1.0
    assert not out["g"][~keep].any(), "dx_hat is not zero on a masked entry"
    dead = case["dead"]
    assert not bits(out["dW"][:, dead]).any() and not bits(out["db"][dead:dead + 1]).any(), "the dead latent's gradient is not +0.0 to the bit"
    # the master after forward_backward: the bias as it was set, to the bit; the weights the column-normalised ones -- the in-place
    # normalisation is a float32 sum of d_p squares, a square root and a division: ((d_p + 2) / 2 + 2) 2^-24 of each element
    if name not in ("after_update",):
        assert np.array_equal(bits(out["params"]["encoder_bias"]), bits(case["b"].numpy())), "forward_backward changed the bias"
        W0 = case["W"].numpy().astype(np.float64)
        norm = np.maximum(np.sqrt((W0 ** 2).sum(0)), 1e-12)
        Wn = W0 / norm[None, :]
        assert (np.abs(out["params"]["decoder.weight"] - Wn) <= ((R.D_P + 2) / 2 + 2) * 2.0 ** -24 * np.abs(Wn)).all(), \
            "the master is not the normalised weights that were set"
    if "twin" in out:
        dW2, db2, p2 = out["twin"]
        assert np.array_equal(bits(out["dW"]), bits(dW2)) and np.array_equal(bits(out["db"]), bits(db2)), "a second engine gives another gradient"
        assert all(np.array_equal(bits(out["params"][k]), bits(p2[k])) for k in p2), "a second engine leaves another master"
    if "gnorm" in out:
        got, want = out["gnorm"]
        assert abs(got - want) <= 8 * 2.0 ** -24 * want, f"clip norm {got!r}, float64 norm of the gradient {want!r}"


@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_inside_the_bounds(runs, name):
    out, ops = runs.get(name), runs.ops(name)
    fwd = R.forward_reference(ops)
    msg = []
    for key in ("c", "g"):
        msg.append(f"{key} {R.worst_ratio(out[key], *fwd[key]).max():.3f}")
        assert not R.violations(out[key], *fwd[key]).any(), f"{name}: " + R.report(key, out[key], *fwd[key])
    print(f"\n{name}: forward worst |difference| / tol   " + "   ".join(msg) + f"   ({ops['guard_moved']} inputs round to -1.0 without being it)")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_backward_inside_the_bounds(runs, name):
    out, ops, plan = runs.get(name), runs.ops(name), R.CASES[name][7]
    ref = R.backward_reference(ops, plan, runs.sums(name))
    msg = []
    for key in ("dW", "db"):
        msg.append(f"{key} {R.worst_ratio(out[key], *ref[key]).max():.3f}")
    print(f"\n{name}: backward worst |difference| / tol   " + "   ".join(msg))
    for key in ("dW", "db"):
        assert not R.violations(out[key], *ref[key]).any(), f"{name}: " + R.report(key, out[key], *ref[key], ref["L"], plan)
    assert ref["L"][runs.case(name)["dead"]] == 0
    if name != "after_update":
        assert ref["L"][runs.case(name)["hot"]] == runs.case(name)["M"]


def test_uniform_switch_leaves_the_forward_alone(runs):
    """debug_flags 83 changes the row partition of the backward and nothing else: latent and dx_hat bitwise as in bal_m3."""
    a, b = runs.get("bal_m3"), runs.get("bal_as_uniform")
    assert np.array_equal(bits(a["c"]), bits(b["c"])) and np.array_equal(bits(a["g"]), bits(b["g"]))
    assert np.array_equal(bits(a["wt"]), bits(b["wt"]))


def test_observers_refuse_other_contexts():
    """sae_l1_backward_plan: TopK and fp8 contexts, M outside [1, max_rows]; sae_debug_read 15: TopK contexts."""
    from freud_amd.engine import EngineError, SaeEngine
    topk = SaeEngine(variant="topk", d_model=256, n_dict=1024, max_rows=256, optimizer="adam", k=8)
    fp8 = SaeEngine(variant="l1", d_model=384, n_dict=256, max_rows=256, optimizer="adam", precision="fp8")
    l1 = SaeEngine(variant="l1", d_model=256, n_dict=256, max_rows=256, optimizer="adam")
    try:
        for eng in (topk, fp8):
            with pytest.raises(EngineError):
                eng.l1_backward_plan(128)
        with pytest.raises(EngineError, match="not an L1 context"):
            topk.debug_read(15, 1024 * 256)
        for M in (0, 257):
            with pytest.raises(EngineError):
                l1.l1_backward_plan(M)
        with pytest.raises(EngineError):
            l1.debug_read(15, 256 * 256 - 1)
        plan = l1.l1_backward_plan(200)      # a GEMM form: no fused grid
        assert plan["form"] >= 2 and plan["grid"] == 0 and plan["balanced"] == 0 and plan["steps"] == 8 and plan["ntiles"] == 2
    finally:
        for eng in (topk, fp8, l1):
            eng.close()
