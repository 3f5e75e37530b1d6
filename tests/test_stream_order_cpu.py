"""The table of stream-taking calls (tests/stream_order_util.py) against the header, without a GPU: every function
of include/gpmpc_mi355x.h with a `void* stream` parameter is named there exactly once, as ordered or as exempt with
a reason, and the cases of tests/test_gpu_stream_order.py run every ordered one in both positions.  A new entry
point fails here until it is classified and given its cases."""

import ast
from pathlib import Path

import stream_order_util as SO

GPU_FILE = Path(__file__).with_name("test_gpu_stream_order.py")
EXEMPT = {"gpmpc_gp_posterior", "gpmpc_preprocess"}


def test_the_parser_sees_the_header():
    fns = SO.stream_functions()
    assert len(fns) == len(set(fns)) == 24, fns   # (today's count: a new entry point changes it, and the table with it)
    assert "gpmpc_solve" in fns and "gpmpc_gp_posterior" in fns and "gpmpc_plant_step" in fns
    # functions without a stream parameter are not the table's business
    assert not {"gpmpc_set_gp", "gpmpc_gp_reserve", "gpmpc_gp_size", "gpmpc_create"} & set(fns)


def test_the_table_names_exactly_the_stream_taking_functions():
    fns = SO.stream_functions()
    assert sorted(SO.TABLE) == sorted(fns), (sorted(set(fns) - set(SO.TABLE)), sorted(set(SO.TABLE) - set(fns)))
    for name, (kind, why) in SO.TABLE.items():
        assert kind in (SO.ORDERED, SO.EXEMPT), name
        assert isinstance(why, str) and len(why) > 10, f"{name}: say what it touches, or why it is exempt"
    assert {n for n, (k, _) in SO.TABLE.items() if k == SO.EXEMPT} == EXEMPT


def test_the_parser_finds_a_new_entry_point(tmp_path):
    """A function added to the header with a stream parameter is seen (whatever the line breaks), and the table
    then no longer matches."""
    extra = ("\ngpmpc_status gpmpc_gp_new_thing(gpmpc_handle* h, int32_t gp_id,\n"
             "                               double* out_dev, void *stream);\n"
             "gpmpc_status gpmpc_no_stream(gpmpc_handle* h, int32_t streams);\n/* void* stream in a comment */\n")
    text = SO.HEADER.read_text().replace("#ifdef __cplusplus\n}\n#endif", extra + "#ifdef __cplusplus\n}\n#endif")
    hdr = tmp_path / "h.h"
    hdr.write_text(text)
    fns = SO.stream_functions(hdr)
    assert "gpmpc_gp_new_thing" in fns and "gpmpc_no_stream" not in fns and len(fns) == 25
    assert sorted(SO.TABLE) != sorted(fns)


def _case_positions():
    """(functions in first position, functions in second position) over the CASES list of the GPU file, read from
    its source: each entry is Case(id, lambda e: (e.<call>(...), e.<call>(...)), ...) or names a pair factory."""
    tree = ast.parse(GPU_FILE.read_text())
    first, second = set(), set()
    method_fn = {}
    util = ast.parse(Path(SO.__file__).read_text())
    for node in ast.walk(util):   # Env.<method> -> the C function its Call names
        if isinstance(node, ast.FunctionDef):
            for sub in ast.walk(node):
                if isinstance(sub, ast.Call) and getattr(sub.func, "id", "") == "Call" and sub.args \
                        and isinstance(sub.args[0], ast.Constant):
                    method_fn.setdefault(node.name, sub.args[0].value)
    factories = {"plant_pair": ("gpmpc_plant_step", "gpmpc_plant_step"), "plant_then_solve": ("gpmpc_plant_step", "gpmpc_solve"),
                 "solve_then_plant": ("gpmpc_solve", "gpmpc_plant_step")}   # (pairs whose second call reads the first's output)
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "id", "") == "Case" and len(node.args) >= 2 \
                and isinstance(node.args[1], ast.Lambda):
            body = node.args[1].body
            if isinstance(body, ast.Tuple):
                names = [method_fn[e.func.attr] for e in body.elts if isinstance(e, ast.Call) and isinstance(e.func, ast.Attribute)]
                assert len(names) == len(body.elts) >= 2, ast.dump(node)[:200]
            else:
                names = factories[body.func.attr]
            first.add(names[0])
            second.add(names[1])
    return first, second


def test_every_ordered_call_is_run_in_both_positions():
    first, second = _case_positions()
    ordered = {n for n, (k, _) in SO.TABLE.items() if k == SO.ORDERED}
    assert ordered - first == set(), f"never the delayed first call: {sorted(ordered - first)}"
    assert ordered - second == set(), f"never the second call: {sorted(ordered - second)}"
