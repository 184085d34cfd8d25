"""Per-point raw of every form of the fused embed + MLP kernels against the float64 restatement (tests/eval_ref.py) on the edge
inputs of tests/eval_cases.py.  Run with `-m gpu` on an MI355X.

Forms (pg_api.hip pick_form), each reached in-process and checked with the launch counters:
  direct16  pg_eval16.hip          bf16 / fp16 at S < 64, and explicit points
  records   pg_eval16r.hip + pg_rayrec.hip   bf16 / fp16 at S >= 64 with set_onchip("records"), or with an activation tap
  onchip    pg_eval16r.hip OC      bf16 / fp16 at S >= 64 with set_onchip("always"), and "auto" at S <= 112
  evalc2    pg_evalc2.hip          fp16c without a tap, S >= 32
  kmajor    pg_eval32.hip          fp32, bf16x3, and fp16c with a tap or on explicit points

Bounds, none taken from a kernel's output (tests/eval_cases.py):
  fp32 / bf16x3 / fp16c   max |raw - float64| <= tol x max(1, |raw|max / 10), tol 4e-5 / 3e-4 / 9e-4; layer-0 tap 2e-5 / 4e-5 / 4e-5
  bf16 / fp16             D = what operand rounding alone does to the case (the restatement with oracle._linear's rounding, on the
                          CPU): max |raw - float64| <= D_max + (4e-2 / 8e-3) x max(1, |raw|max / 10), and RMS <= 2 D_rms
Far-skip and empty-skip stay at their defaults; the restatement never masks.

Worst measured / bound on an MI355X over the 400 raw and 48 tap comparisons of this file (max-abs of raw; RMS; layer-0 tap):
  direct16  bf16 0.53 / 0.51          fp16 0.41 / 0.50
  records   bf16 0.55 / 0.58          fp16 0.44 / 0.58 / tap 0.14
  onchip    bf16 0.55 / 0.58          fp16 0.44 / 0.58
  evalc2    fp16c 0.37
  kmajor    fp32 0.69 / tap 0.82      bf16x3 0.32      fp16c 0.37 / tap 0.40
The parent's pg_evalc2.hip missed test_cutoffs at tau_d = -4 by 2.0 in raw (bound 2e-3): the far-skip radius assumed tau > 0.
"""
import pytest
import torch

from posegen_amd import PREC_BY_NAME
from tests import eval_cases as ec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIXTEEN = ("bf16", "fp16")
WORST = {}          # (form, precision) -> the largest measured / bound ratio of this session, printed with every check


@pytest.fixture(scope="module")
def renderers():
    from posegen_amd.raycaster import HipRayCaster
    cache = {}

    def get(model):
        if model not in cache:
            cfg, wc, wf = ec.model(model)
            cache[model] = HipRayCaster.from_weights(cfg, wc, wf, ec.TAU_MODEL, ec.TAU_MODEL, device=DEV, precision="bf16")
        return cache[model].renderer
    yield get
    for c in cache.values():
        c.renderer.close()


def _form_setup(form, prec, case):
    """(set_onchip mode, tap, record launches expected) of a form; refuses a (form, precision, case) the form does not run"""
    S = None if case.pts is not None else case.S
    if form == "direct16":
        assert prec in SIXTEEN and (S is None or 32 <= S < 64)
        return "auto", False, 0
    if form in ("records", "records_tap", "records_auto"):
        assert prec in SIXTEEN and S >= 64 and (form != "records_auto" or S > 112)
        # (a tap needs records whatever the mode)
        return {"records": ("records", False, 1), "records_tap": ("always", True, 1), "records_auto": ("auto", False, 1)}[form]
    if form in ("onchip", "onchip_auto"):
        assert prec in SIXTEEN and S >= 64 and (form == "onchip" or S <= 112)
        return ("always" if form == "onchip" else "auto"), False, 0
    if form == "evalc2":
        assert prec == "fp16c" and S >= 32
        return "auto", False, 0
    if form in ("kmajor", "kmajor_tap"):
        assert prec in ("fp32", "bf16x3") or (prec == "fp16c" and (form == "kmajor_tap" or S is None))
        return "auto", form == "kmajor_tap", 0
    raise AssertionError(form)


def _launch(r, case, which, prec, onchip, tap):
    """the case through stage_eval / query_density with the case's embedder state; every setting put back"""
    dbg = None
    try:
        r.set_precision(PREC_BY_NAME[prec])
        r.set_onchip(onchip)
        r.set_embedder(0, case.tau_v, case.cutoff_v)
        r.set_embedder(1, case.tau_d, case.cutoff_d)
        r.profile_enable(True)
        r.profile_read(); r.profile_read_aux()
        if case.pts is not None:
            raw = r.query_density(torch.tensor(case.pts), torch.tensor(case.skts), which)
        else:
            cams = None if case.cams is None else torch.tensor(case.cams)
            out = r.stage_eval(which, torch.tensor(case.ray_batch), torch.tensor(case.z), torch.tensor(case.skts), cams=cams, want_dbg=tap)
            raw, dbg = out if tap else (out, None)
        torch.cuda.synchronize()
        launches, _, n_pts = r.profile_read()
        recs, _ = r.profile_read_aux()
        raw = raw.cpu().double()
        dbg = None if dbg is None else dbg.cpu().double()
    finally:
        r.profile_enable(False)
        r.set_onchip("auto")
        r.set_embedder(0, ec.TAU_MODEL)
        r.set_embedder(1, ec.TAU_MODEL)
        r.set_precision("bf16")
    return raw, dbg, launches, recs, n_pts


def check(renderers, case, which, form, prec):
    """One launch of `case` in `form` / `prec`: the form ran (counters), raw (and the tap) within the precision's bound."""
    onchip, tap, want_recs = _form_setup(form, prec, case)
    raw, dbg, launches, recs, n_pts = _launch(renderers(case.model), case, which, prec, onchip, tap)
    assert (launches, recs, n_pts) == (1, want_recs, case.n_points), (case.name, form, prec, launches, recs, n_pts)
    ref = ec.reference(case, which)
    want = ref["raw"][..., 3:4].reshape(raw.shape) if case.pts is not None else ref["raw"]
    assert torch.isfinite(raw).all(), (case.name, form, prec)
    err = raw - want
    emax, erms, scale = float(err.abs().max()), float(err.pow(2).mean().sqrt()), float(want.abs().max())
    tag = f"[{case.name} net {which} {form} {prec}]"
    ratios = []
    if prec in SIXTEEN:
        y = ec.yardstick(case, which, prec)
        bmax, brms = ec.bound_16bit(prec, y), ec.RMS_FACTOR * y["rms"]
        print(f"{tag} raw max {emax:.3e} <= {bmax:.3e} (D_max {y['max']:.3e}); rms {erms:.3e} <= {brms:.3e}; |raw| max {scale:.1f}")
        ratios += [emax / bmax, erms / brms]
        ok = emax <= bmax and erms <= brms
    else:
        bmax = ec.bound_exact(prec, scale)
        print(f"{tag} raw max {emax:.3e} <= {bmax:.3e}; |raw| max {scale:.1f}")
        ratios.append(emax / bmax)
        ok = emax <= bmax
    if tap:
        e0 = float((dbg.reshape(ref["pre0"].shape) - ref["pre0"]).abs().max())
        b0 = ec.yardstick(case, which, prec)["max0"] + ec.EMUL_TOL[prec] if prec in SIXTEEN else ec.EXACT_TAP_TOL[prec]
        print(f"{tag} layer-0 pre-activation max {e0:.3e} <= {b0:.3e} (|pre0| max {float(ref['pre0'].abs().max()):.1f})")
        ratios.append(e0 / b0)
        ok = ok and e0 <= b0
    key = (form.split("_")[0], prec)
    WORST[key] = max(WORST.get(key, 0.0), *ratios)
    print(f"{tag} worst measured / bound so far for {key}: {WORST[key]:.3f}")
    assert ok, tag
    return raw


def forms_for(S, taps=True):
    """every (form, precision) that runs rays of S samples"""
    out = [("kmajor", "fp32"), ("kmajor", "bf16x3")] + ([("kmajor_tap", "fp16c"), ("kmajor_tap", "fp32")] if taps else [])
    if S >= 32:
        out.append(("evalc2", "fp16c"))
    if 32 <= S < 64:
        out += [("direct16", p) for p in SIXTEEN]
    if S >= 64:
        out += [(f, p) for f in ("records", "onchip") for p in SIXTEEN]
        out.append(("onchip_auto" if S <= 112 else "records_auto", "fp16"))     # "auto": on chip up to 112 samples per ray
        if taps:
            out.append(("records_tap", "fp16"))
    return out


# ---------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("n,S", [(n, S) for S in (16,) + ec.SEAM_S for n in ec.SEAM_N])
def test_seams(renderers, n, S):
    """Per-ray poses (the PP variants), a frame code per ray (FC), rays / poses / codes changing inside waves and passes, ragged
    last pass; S = 16 (k-major only), 32 / 33 (direct16, evalc2), 64 / 65 (a 256-point pass over 5 rays), 112 / 113 (either side
    of the "auto" switch from on-chip to records).  The coarse net on the 7-ray launches, the fine net on the 13-ray ones.
    Worst measured / bound on an MI355X: see DESIGN.md "eval point tests"."""
    case = ec.seams(n, S)
    which = int(n == 13)
    for form, prec in forms_for(S, taps=(n == 13)):
        check(renderers, case, which, form, prec)


@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("tau_v,tau_d", ec.CUTOFF_TAUS)
def test_cutoffs(renderers, tau_v, tau_d, S):
    """Per-joint cutoffs, different for the two embedders, tau in {4, 79.6, 400} and tau_d = -4: a slot-for-joint mix-up, the
    two embedders' cutoffs exchanged or a dropped in-range limb moves raw by 2 .. 9 (tests/test_eval_ref_host.py).  At (79.6, 400)
    two rays pass a wrist at the far-skip radius x (1 -+ 2^-18).  tau_d = -4: the far-skip radius cutoff + 24 / (tau log2 e)
    assumed tau > 0 -- the masks dropped limbs whose view weight is ~1; the radius is now infinite for tau <= 0."""
    case = ec.cutoffs(tau_v, tau_d, S)
    for which in (0, 1):
        for form, prec in forms_for(S, taps=(which == 0)):
            check(renderers, case, which, form, prec)


@pytest.mark.parametrize("S", [32, 64])
def test_on_joint(renderers, S):
    """A sample exactly on a joint (q = 0 in fp32 in both forms of the transform; rsq(max(d^2, 1e-24)) against F.normalize) and
    its neighbours at 2^-10 .. 2^-4: finite, and within the bounds like every other point."""
    case = ec.on_joint(S)
    r, k = case.note["ray"], case.note["sample"]
    for which in (0, 1):
        want = ec.reference(case, which)["raw"][r, k]
        for form, prec in forms_for(S, taps=(which == 1)):
            raw = check(renderers, case, which, form, prec)
            print(f"    on the joint: |raw - float64| = {float((raw[r, k] - want).abs().max()):.3e}")


@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("layout", ["all", "first", "last"])
def test_all_far(renderers, layout, S):
    """Rays that miss every limb's radius (the weight ring starts fully masked): every ray; the whole first pass only; only the
    last, ragged pass.  raw of the far rays is the net's empty-space output."""
    case = ec.all_far(layout, S)
    for form, prec in forms_for(S, taps=False):
        check(renderers, case, 0, form, prec)


@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("one_element", [False, True])
def test_codes(renderers, one_element, S):
    """Frame-code indices -1 (the mean row), 0 and n_codes - 1 mixed per ray, and a one-element `cams`; both nets."""
    case = ec.codes(one_element, S)
    for which in (0, 1):
        for form, prec in forms_for(S, taps=(which == 1 and not one_element)):
            check(renderers, case, which, form, prec)


@pytest.mark.parametrize("S", [32, 64])
def test_ties(renderers, S):
    """Ascending depths with runs of equal values, and a ray whose depths are all one value (first == last: the segment the
    pass masks are made from is a point)."""
    case = ec.ties(S)
    for form, prec in forms_for(S, taps=False):
        check(renderers, case, 1, form, prec)


@pytest.mark.parametrize("count", [1, 129, 257])
def test_points(renderers, count):
    """query_density on explicit points: on a joint, at the far-skip radius x (1 -+ 2^-18), far away, around the body; sigma of
    both nets (direct16 for bf16 / fp16, the k-major kernel for fp32 / bf16x3 / fp16c)."""
    case = ec.points(count)
    for which in (0, 1):
        for prec in SIXTEEN:
            check(renderers, case, which, "direct16", prec)
        for prec in ("fp32", "bf16x3", "fp16c"):
            check(renderers, case, which, "kmajor", prec)
