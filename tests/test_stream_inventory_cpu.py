"""Every function of mlmc_amd that can hand a CUDA tensor to the C library is exercised by tests/test_gpu_stream_order.py or
is exempt for a stated reason (no GPU needed: the sources are parsed, tests/stream_cases.py touches no device at import).

A function counts when it calls `.data_ptr()`, or `_lib.ptr(x)` with an x that is not provably a NumPy array: a name is provably
NumPy when every assignment to it in the function is a call of `np.*` / `_lib.as_f64` (or a method of such a call), a literal
None, or another provably-NumPy name.  Parameters, attributes, subscripts and everything made by torch are not.  Nested
functions belong to the outermost function that holds them.  A device entry added later fails this test until it has an
inventory row (or an exemption with a reason)."""
import ast
import os

from tests import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mlmc_amd")


def _numpy_call(node, numpy_names):
    """the expression is a NumPy array (or None) for certain"""
    if isinstance(node, ast.Constant) and node.value is None:
        return True
    if isinstance(node, ast.Name):
        return node.id in numpy_names
    if isinstance(node, ast.IfExp):
        return _numpy_call(node.body, numpy_names) and _numpy_call(node.orelse, numpy_names)
    if isinstance(node, ast.Call):
        f = node.func
        if isinstance(f, ast.Attribute):
            if isinstance(f.value, ast.Name) and f.value.id == "np":
                return True
            if isinstance(f.value, ast.Name) and f.value.id == "_lib" and f.attr == "as_f64":
                return True
            return _numpy_call(f.value, numpy_names)           # a method of a NumPy array: reshape, copy, astype ...
    return False


def _assignments(fn):
    """name -> the list of expressions assigned to it anywhere in the function (None stands for 'not an expression we follow')"""
    out = {}
    params = set()
    for node in ast.walk(fn):
        if isinstance(node, (ast.FunctionDef, ast.Lambda)):
            a = node.args
            for arg in a.posonlyargs + a.args + a.kwonlyargs + [x for x in (a.vararg, a.kwarg) if x is not None]:
                params.add(arg.arg)
        elif isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Name):
                    out.setdefault(t.id, []).append(node.value)
                else:
                    for sub in ast.walk(t):
                        if isinstance(sub, ast.Name):
                            out.setdefault(sub.id, []).append(None)
        elif isinstance(node, (ast.AugAssign, ast.AnnAssign)) and isinstance(node.target, ast.Name):
            out.setdefault(node.target.id, []).append(None)
        elif isinstance(node, (ast.For, ast.comprehension)):
            for sub in ast.walk(node.target):
                if isinstance(sub, ast.Name):
                    out.setdefault(sub.id, []).append(None)
        elif isinstance(node, ast.withitem) and node.optional_vars is not None:
            for sub in ast.walk(node.optional_vars):
                if isinstance(sub, ast.Name):
                    out.setdefault(sub.id, []).append(None)
    for p in params:
        out.setdefault(p, []).append(None)
    return out


def _numpy_names(fn):
    assigned = _assignments(fn)
    known = set()
    for _ in range(4):                                            # names defined from names: a few rounds reach the fixed point
        for name, values in assigned.items():
            if name not in known and all(v is not None and _numpy_call(v, known) for v in values):
                known.add(name)
    return known


def hands_over_device_memory(fn):
    known = _numpy_names(fn)
    for node in ast.walk(fn):
        if not isinstance(node, ast.Call) or not isinstance(node.func, ast.Attribute):
            continue
        f = node.func
        if f.attr == "data_ptr":
            return True
        if f.attr == "ptr" and isinstance(f.value, ast.Name) and f.value.id == "_lib" and node.args:
            if not _numpy_call(node.args[0], known):
                return True
    return False


def device_functions():
    """'module.path:Qualified.name' of every outermost function or method of mlmc_amd that hands over possibly-CUDA memory"""
    found = []
    for base, _, files in os.walk(PKG):
        for name in sorted(files):
            if not name.endswith(".py"):
                continue
            path = os.path.join(base, name)
            mod = os.path.relpath(path, ROOT)[:-3].replace(os.sep, ".")
            with open(path) as fh:
                tree = ast.parse(fh.read(), path)

            def visit(body, prefix):
                for node in body:
                    if isinstance(node, ast.ClassDef):
                        visit(node.body, prefix + node.name + ".")
                    elif isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                        if hands_over_device_memory(node):
                            found.append("{}:{}{}".format(mod, prefix, node.name))
            visit(tree.body, "")
    return sorted(found)


def test_detector_on_small_sources():
    """the rule itself: data_ptr, _lib.ptr of a parameter and of a torch tensor count; _lib.ptr of NumPy arrays does not"""
    src = '''
def a(x):
    return x.data_ptr()
def b(x):
    q = _lib.as_f64(x)
    out = np.empty(3)
    call(_lib.ptr(q), _lib.ptr(out), _lib.ptr(None))
def c(x):
    call(_lib.ptr(x))
def d(n):
    t = torch.empty(n)
    call(_lib.ptr(t))
def e(x):
    y = np.asarray(x).reshape(-1)
    z = y
    call(_lib.ptr(z))
def f(x):
    y = np.asarray(x)
    if flag:
        y = x.contiguous()
    def inner():
        call(_lib.ptr(y))
'''
    fns = {n.name: n for n in ast.parse(src).body}
    assert {k for k, v in fns.items() if hands_over_device_memory(v)} == {"a", "c", "d", "f"}


def inventory_problems(rows, found):
    """what is wrong with an inventory, as sentences (none: every device function is covered or exempt, every required row there)"""
    out = []
    covered = {}
    for row in rows:
        for name in row.covers:
            covered.setdefault(name, []).append(row.name)
        if not (callable(row.build) and callable(row.run) and callable(row.flat) and row.covers):
            out.append("row {} is incomplete".format(row.name))
    exempt = set(sc.EXEMPT)
    if not all(isinstance(r, str) and len(r) > 20 for r in sc.EXEMPT.values()):
        out.append("an exemption needs its reason")
    names = [r.name for r in rows]
    if len(names) != len(set(names)):
        out.append("two rows share a name")
    if set(names) != set(sc.REQUIRED_ROWS):
        out.append("rows missing: {}; rows not in REQUIRED_ROWS: {}".format(sorted(set(sc.REQUIRED_ROWS) - set(names)),
                                                                           sorted(set(names) - set(sc.REQUIRED_ROWS))))
    stale = (set(covered) | exempt) - found
    if stale:
        out.append("inventoried or exempt, but no longer a device function of mlmc_amd: {}".format(sorted(stale)))
    if set(covered) & exempt:
        out.append("both inventoried and exempt: {}".format(sorted(set(covered) & exempt)))
    missing = found - set(covered) - exempt
    if missing:
        out.append("these functions hand CUDA memory to the library and have neither an inventory row in tests/stream_cases.py nor an "
                   "exemption: {}".format(sorted(missing)))
    return out


def test_every_device_function_is_inventoried_or_exempt():
    assert inventory_problems(sc.INVENTORY, set(device_functions())) == []


def test_removing_any_row_is_noticed():
    found = set(device_functions())
    for drop in range(len(sc.INVENTORY)):
        rest = [r for i, r in enumerate(sc.INVENTORY) if i != drop]
        assert inventory_problems(rest, found), sc.INVENTORY[drop].name


def test_a_new_device_function_is_noticed():
    found = set(device_functions()) | {"mlmc_amd.engine:some_new_entry"}
    assert any("some_new_entry" in p for p in inventory_problems(sc.INVENTORY, found))
