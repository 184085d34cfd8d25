"""The case table of tests/test_gpu_streams.py against include/posegen_hip.h (no GPU): every entry point that takes a stream is
covered by exactly one case or, for pg_stage_* only, by a named case that runs the same launcher; nothing is listed that the
header lacks; every claim about what synchronises or is asynchronous quotes the header."""
import os
import re

from tests import stream_harness as sh

TEXT = sh.header_text()
ENTRY_POINTS = sh.stream_entry_points(TEXT)
# the header's comments as running text: line breaks and the ` * ` of comment continuation lines become one space
PROSE = re.sub(r"\s*\n\s*\*?\s*", " ", TEXT)


def test_the_parser_finds_the_stream_taking_entry_points():
    assert len(ENTRY_POINTS) == len(set(ENTRY_POINTS)) == 45, sorted(ENTRY_POINTS)
    for name in ("pg_render_rays", "pg_train_backward_pose", "pg_stage_scene_composite", "pg_grad_norms", "pg_load_weights_device"):
        assert name in ENTRY_POINTS
    for name in ("pg_render_frames", "pg_load_weights", "pg_plan_frames", "pg_create"):        # no stream parameter
        assert name not in ENTRY_POINTS


def test_every_stream_taking_entry_point_is_covered_exactly_once():
    named = [e for eps in sh.CASES.values() for e in eps]
    for e in ENTRY_POINTS:
        n = named.count(e) + (e in sh.COVERED_BY)
        assert n == 1, f"{e} is named by {named.count(e)} cases and {int(e in sh.COVERED_BY)} COVERED_BY entries; exactly one expected"


def test_the_tables_name_nothing_the_header_lacks():
    for table in (sh.CASES, sh.VARIANTS):
        for case, eps in table.items():
            assert eps, case
            for e in eps:
                assert e in ENTRY_POINTS, f"case {case} names {e}, which the header does not declare with a stream"
    assert not set(sh.CASES) & set(sh.VARIANTS)
    for case, eps in sh.VARIANTS.items():                   # a variant adds a path of an entry point that a case already names
        for e in eps:
            assert any(e in v for v in sh.CASES.values()), (case, e)


def _csrc(name):
    with open(os.path.join(sh.REPO, "posegen_amd", "csrc", name)) as f:
        return f.read()


def _function_body(src, name):
    """the text of the C function `name` (from its definition to the next function definition at column 0)"""
    m = re.search(rf"^int {name}\(", src, flags=re.M)
    assert m, name
    end = re.search(r"^}\n", src[m.start():], flags=re.M)
    return src[m.start():m.start() + end.end()]


def test_covered_by_holds_stage_entry_points_only_and_names_a_shared_launcher():
    """A COVERED_BY reason starts with the launcher's name; the stage entry point AND an entry point of the named case both call
    that symbol in pg_api.hip with their `stream` argument -- a launcher that does not exist, or that the stage entry point does
    not go through, is refused."""
    api = _csrc("pg_api.hip")
    for e, (case, reason) in sh.COVERED_BY.items():
        assert e.startswith("pg_stage_") and e in ENTRY_POINTS, e
        assert case in sh.CASES or case in sh.VARIANTS, (e, case)
        assert "\n" not in reason
        launcher = re.match(r"(\w+)", reason).group(1)
        assert re.search(rf"\b{launcher}\(", _function_body(api, e)), f"{e} does not call {launcher}"
        callers = len(re.findall(rf"\b{launcher}\([^;]*\bstream\b", api))
        assert callers >= 2, f"{launcher} is called with a stream in {callers} place(s) of pg_api.hip: nothing shares it with {e}"
    # the render calls reach the same launchers: render_rays_impl is what pg_render_rays and pg_render_rays_train run
    for launcher in ("pg_launch_sample_coarse", "launch_eval", "pg_launch_composite"):
        assert len(re.findall(rf"\b{launcher}\(", api)) >= 3, launcher


def test_every_documented_asynchronous_entry_point_has_its_pending_flag_asserted():
    """an entry point of ASYNCHRONOUS sits in a case all of whose entry points are asynchronous, or ends at a probe of a mixed chain"""
    asserted = sh.asserted_pending()
    for e in sh.ASYNCHRONOUS:
        if e not in sh.SYNCHRONISES:
            assert e in asserted, f"{e} is documented as asynchronous, but no case asserts that the delay is pending after it"
    for case, eps in sh.PROBES.items():
        assert case in sh.CASES and set(eps) <= set(sh.CASES[case]), case


def test_synchronises_and_asynchronous_quote_the_header():
    for table in (sh.SYNCHRONISES, sh.ASYNCHRONOUS):
        for e, quote in table.items():
            assert e in ENTRY_POINTS, e
            assert quote in PROSE, f"{e}: the header does not say {quote!r}"
    assert not set(sh.SYNCHRONISES) & set(sh.ASYNCHRONOUS)
    for e, quote in sh.SYNCHRONISES.items():
        assert "synchronises" in quote and e in quote, (e, quote)
    assert not sh.must_stay_pending(sh.CASES["grid_mesh"]) and sh.must_stay_pending(sh.CASES["render_rays_fp32"])


def _cases_run_by_the_gpu_module():
    """the case names the GPU module hands to the harness: the second argument of its check(...) and _train_case(...) calls where
    that is a literal, and the keys of RAY_CASES, which test_ray_rendering is parametrised over -- from the syntax tree, so that a
    name in a comment or a docstring does not count"""
    import ast
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_streams.py")) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ("check", "_train_case") and len(node.args) > 1:
            arg = node.args[1]
            if isinstance(arg, ast.Constant) and isinstance(arg.value, str):
                names.add(arg.value)
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "RAY_CASES" for t in node.targets):
            names.update(k.value for k in node.value.keys)
    return names


def test_every_case_has_a_test_in_the_gpu_module():
    run = _cases_run_by_the_gpu_module()
    listed = set(sh.CASES) | set(sh.VARIANTS)
    assert run == listed, (sorted(listed - run), sorted(run - listed))


def test_removing_an_entry_point_from_the_table_is_noticed():
    """the coverage check is not vacuous: without its case an entry point is reported"""
    cases = {k: v for k, v in sh.CASES.items() if k != "grad_norms"}
    named = [e for eps in cases.values() for e in eps]
    assert [e for e in ENTRY_POINTS if named.count(e) + (e in sh.COVERED_BY) != 1] == ["pg_grad_norms"]
