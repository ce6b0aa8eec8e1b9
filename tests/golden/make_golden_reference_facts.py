"""Generates tests/golden/reference_facts.json: what the CPU tests check about the REFERENCE's scripts/splatam.py and its
cpu_baseline leg, recorded where the reference tree is present so that the tests need no copy of it (no source text is stored):

  * ``loop_lines``: the line numbers of the loop statements tests/test_gpu_plugin.py restates (tests/test_plugin_cpu.py checks their order);
  * ``rgbd_slam``: how ``rgbd_slam`` looks up the names splatam_amd.plugin replaces (module globals, not locals) and the shape of every
    call of them inside it -- positional argument count and keyword names, from the source's syntax tree -- which the adapters'
    signatures must bind;
  * ``cpu_baseline_scene_a``: the first loss of bench.py's cpu_baseline leg through the reference's own modules on
    tests/test_cpu_baseline_reference.py's scene (the mirror's loss of the same inputs is held to it).

The extraction functions are also what the tests call to check the record against the reference wherever it is present.

Run:  python tests/golden/make_golden_reference_facts.py     (needs the reference tree: SPLAT_REFERENCE_DIR, as bench.py)
"""
import ast
import hashlib
import json
import os
import re
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_facts.json")
PLUGIN_NAMES = ("get_loss", "initialize_optimizer", "add_new_gaussians", "prune_gaussians", "densify")

# (key, pattern) in the order the loop executes them; searched after the optimizer's line, up to the last line of the loop
TRACKING = (("get_loss", r"loss, variables, losses = get_loss\(params, tracking_curr_data, variables, iter_time_idx"),
            ("backward", r"loss\.backward\(\)"), ("step", r"optimizer\.step\(\)"), ("zero_grad", r"optimizer\.zero_grad\(set_to_none=True\)"),
            ("best_candidate", r"if loss < current_min_loss"))
MAPPING = (("get_loss", r"loss, variables, losses = get_loss\(params, iter_data, variables, iter_time_idx"),
           ("backward", r"loss\.backward\(\)"), ("prune_gaussians", r"params, variables = prune_gaussians\(params, variables, optimizer, iter"),
           ("step", r"optimizer\.step\(\)"), ("zero_grad", r"optimizer\.zero_grad\(set_to_none=True\)"))
TRACKING_OPTIMIZER = (r"optimizer = initialize_optimizer\(params, config\['tracking'\]\['lrs'\], tracking=True\)", 670, 690, 745)
MAPPING_OPTIMIZER = (r"optimizer = initialize_optimizer\(params, config\['mapping'\]\['lrs'\], tracking=False\)", 800, 830, 895)


def reference_dir():
    sys.path.insert(0, ROOT)
    import bench
    return bench.REFERENCE_DIR


def loop_lines(src):
    """Line numbers (1-based) of the definitions the adapters mirror and of the loop statements, from the source's lines."""
    def first(pattern, lo, hi):
        for i in range(lo - 1, hi):
            if re.search(pattern, src[i]):
                return i + 1
        raise AssertionError(f"{pattern!r} not found in lines {lo}-{hi}")

    def loop(optimizer, statements):
        pattern, lo, hi, end = optimizer
        opt = first(pattern, lo, hi)
        return dict([("optimizer", opt)] + [(k, first(p, opt, end)) for k, p in statements])
    return {"get_loss_def": first(r"def get_loss\(params, curr_data, variables, iter_time_idx, loss_weights, use_sil_for_loss,", 1, len(src)),
            "initialize_optimizer_def": first(r"def initialize_optimizer\(params, lrs_dict, tracking\):", 1, len(src)),
            "tracking": loop(TRACKING_OPTIMIZER, TRACKING), "mapping": loop(MAPPING_OPTIMIZER, MAPPING)}


def rgbd_slam_facts(text):
    """How the module-level ``rgbd_slam`` resolves PLUGIN_NAMES (its code object, compiled from its own source segment) and every call
    of them in it (source order): name, positional argument count, keyword names."""
    tree = ast.parse(text)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "rgbd_slam")
    mod = compile(ast.Module(body=[fn], type_ignores=[]), "rgbd_slam", "exec")
    code = next(c for c in mod.co_consts if isinstance(c, types.CodeType) and c.co_name == "rgbd_slam")
    calls = sorted((n for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in PLUGIN_NAMES),
                   key=lambda n: (n.lineno, n.col_offset))
    return {"module_level": True,
            "global_lookup": {k: (k in code.co_names and k not in code.co_varnames and k not in code.co_freevars) for k in PLUGIN_NAMES},
            "calls": [{"name": n.func.id, "args": len(n.args), "keywords": [k.arg for k in n.keywords]} for n in calls]}


def cpu_baseline_scene_a():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    import test_cpu_baseline_reference as T
    params, frames, mirror_loss = T._scene_a()
    out = bench.cpu_baseline_reference("A", params, frames, budget_s=5.0, max_iters=1)
    assert out is not None and out["kind"] == "reference glue + oracle", out
    return {"first_loss": out["first_loss"], "mirror_loss_when_recorded": mirror_loss}


def main():
    ref = reference_dir()
    path = os.path.join(ref, "scripts", "splatam.py")
    text = open(path).read()
    facts = {"reference_splatam_py_sha256": hashlib.sha256(text.encode()).hexdigest(),
             "loop_lines": loop_lines(text.splitlines()), "rgbd_slam": rgbd_slam_facts(text),
             "cpu_baseline_scene_a": cpu_baseline_scene_a()}
    with open(OUT, "w") as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(facts))


if __name__ == "__main__":
    main()
