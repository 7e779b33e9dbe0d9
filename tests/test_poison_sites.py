"""CPU: the exclusion table of tests/poison.py is complete. Every torch.empty / empty_like / new_empty site of the package
whose buffer the poison helper does not fill (an integer or byte dtype outside the weight-plane producers) must be listed
in poison.UNPOISONED with a reason, so that a new integer scratch buffer is reviewed into the table (or made a float) and
the table names no site that no longer exists."""
import ast
import glob
import os

import poison
from conftest import ROOT

PKG = os.path.join(ROOT, "multishiftseg_amd")
FLOAT_DTYPES = {"float32", "float", "float64", "double", "float16", "half", "bfloat16"}
EMPTY_FUNCS = {"empty", "empty_like", "new_empty"}


def _dtype_name(node):
    """'float32' for torch.float32 / float32, None when the expression is not a plain dtype name."""
    if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "torch":
        return node.attr
    if isinstance(node, ast.Name):
        return node.id
    return None


def _is_torch_empty(call):
    f = call.func
    if not isinstance(f, ast.Attribute) or f.attr not in EMPTY_FUNCS:
        return False
    if f.attr == "new_empty":
        return True
    return isinstance(f.value, ast.Name) and f.value.id == "torch"


class _Sites(ast.NodeVisitor):
    """(module, function, variable, dtype) of every allocation; dtype None = inherited from the argument (empty_like /
    new_empty without dtype=), resolved through a same-function `name = torch.empty(..., dtype=...)` where there is one."""

    def __init__(self, module):
        self.module = module
        self.func = ["<module>"]
        self.sites = []
        self.assigned = {}          # (function, name) -> dtype of an explicit allocation

    def visit_FunctionDef(self, node):
        self.func.append(node.name)
        self.generic_visit(node)
        self.func.pop()

    visit_AsyncFunctionDef = visit_FunctionDef

    def _target(self, stmt, call):
        if isinstance(stmt, ast.Assign):
            tgts = stmt.targets[0]
            if isinstance(tgts, ast.Name):
                return tgts.id
            if isinstance(tgts, ast.Tuple) and isinstance(stmt.value, ast.Tuple):
                for t, v in zip(tgts.elts, stmt.value.elts):
                    if call in ast.walk(v) and isinstance(t, ast.Name):
                        return t.id
        return None

    def visit_Assign(self, node):
        for call in [n for n in ast.walk(node.value) if isinstance(n, ast.Call) and _is_torch_empty(n)]:
            self._record(call, self._target(node, call))
        self.generic_visit(node)

    def visit_Call(self, node):
        if _is_torch_empty(node) and not getattr(node, "_seen", False):
            self._record(node, None)
        self.generic_visit(node)

    def _record(self, call, var):
        call._seen = True
        dtype = next((_dtype_name(k.value) for k in call.keywords if k.arg == "dtype"), None)
        if dtype is None and call.func.attr == "empty":
            dtype = "float32"                                   # torch's default dtype
        if dtype is None:                                       # inherited: empty_like(x) / x.new_empty(...)
            src = call.args[0] if call.func.attr == "empty_like" and call.args else call.func.value
            if isinstance(src, ast.Name):
                dtype = self.assigned.get((self.func[-1], src.id))
        if var is not None and dtype is not None:
            self.assigned[(self.func[-1], var)] = dtype
        self.sites.append((self.module, self.func[-1], var, dtype))


def _all_sites():
    sites = []
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        v = _Sites(os.path.splitext(os.path.basename(path))[0])
        v.visit(ast.parse(open(path).read(), path))
        sites += v.sites
    return sites


def _poisoned(module, func, dtype):
    if dtype is None or dtype in FLOAT_DTYPES:      # inherited dtypes are float unless resolved otherwise (checked at run time too)
        return True
    return dtype == "uint8" and module == "kernels" and func in poison.PLANE_PRODUCERS


def test_every_unpoisoned_allocation_is_listed():
    sites = _all_sites()
    assert len(sites) > 100                                  # the scan sees the package
    table = {(m, f, v) for m, f, v, _ in poison.UNPOISONED}
    missing = sorted({(m, f, str(v), d) for m, f, v, d in sites if not _poisoned(m, f, d) and (m, f, v) not in table})
    assert not missing, f"integer / byte buffers that tests/poison.py does not poison and does not list in UNPOISONED: {missing}"


def test_the_table_lists_only_live_unpoisoned_sites():
    # an inherited dtype (empty_like of a buffer made elsewhere) may be an integer one: such a site may be listed
    live = {(m, f, v) for m, f, v, d in _all_sites() if d is None or not _poisoned(m, f, d)}
    stale = [(m, f, v) for m, f, v, _ in poison.UNPOISONED if (m, f, v) not in live]
    assert not stale, f"UNPOISONED entries with no unpoisoned allocation site behind them: {stale}"
    assert all(r.strip() for *_, r in poison.UNPOISONED)


def test_plane_producers_allocate_uint8_planes():
    """The 0xFF fill follows the allocating function's name: every producer still allocates its planes as uint8."""
    got = {f for m, f, _, d in _all_sites() if m == "kernels" and d == "uint8"}
    assert poison.PLANE_PRODUCERS <= got, poison.PLANE_PRODUCERS - got
