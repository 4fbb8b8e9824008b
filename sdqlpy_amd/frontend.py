"""Front end: Python AST of an @sdql_compile function -> scan-operator IR.

The reference does the same job in src/sdqlpy/lib/sdql_compiler.py (an ast.NodeVisitor that prints
IR-constructor text: sum 43-82, joinBuild 162-187, joinProbe 189-210, and/or 277-292, if/else
223-231) followed by type inference and a C++ printer.  This front end is written from scratch for
the HIP backend: it produces one `ScanOp` per table-scanning `sum` / `joinBuild` / `joinProbe` —
exactly the loops the reference's generator emits for `SumExpr` nodes over database tables
(src/sdqlpy/lib/sdql_ir_cpp_generator_par.py:188) — plus a `FinalizeOp` for the trailing
"reshape (key, value) into one record" sum (K-F, generator 520-568).  planner.py then maps each
operator onto a pattern call of include/sdqh.h; an operator outside the backend's vocabulary raises
`UnsupportedQuery` with the offending source line (never a silent fallback).
"""
import ast
import inspect
import textwrap


class UnsupportedQuery(NotImplementedError):
    pass


# ---- expression IR ------------------------------------------------------------------------------
class Expr:
    def shape(self, names):
        """Canonical string with columns replaced by c0, c1, ... in first-occurrence order."""
        raise NotImplementedError


class Col(Expr):
    """A field of the scanned row (`p[0].x`, `probeDictKey.x`)."""
    def __init__(self, name):
        self.name = name

    def shape(self, names):
        key = ("col", self.name)
        if key not in names:
            names.append(key)
        return "c%d" % names.index(key)

    def __repr__(self):
        return "Col(%s)" % self.name


class PayloadField(Expr):
    """A field of the entry matched by a lookup (`indexedDictValue.x`, `tbl[key].x`); field None =
    the entry's whole value (a scalar payload)."""
    def __init__(self, lookup, field):
        self.lookup, self.field = lookup, field

    def shape(self, names):
        key = ("payload", self.lookup.dict_name, repr(self.lookup.key), self.field)
        if key not in names:
            names.append(key)
        return "c%d" % names.index(key)

    def __repr__(self):
        return "Payload(%s[%r].%s)" % (self.lookup.dict_name, self.lookup.key, self.field)


DISTINCT_FIELD = "distinct"     # the one value field of a dictionary of sets as the executor keeps it: the size of each set


class DistinctCount(PayloadField):
    """`dictSize(tbl[key])` where `tbl = T.sum(lambda p: {k: vector({v})})`: the number of DISTINCT v among the rows of key k (the
    reference's Python mode keeps such vectors as sets: `vector.__add__` is a set union, lib/sdql_lib.py).  An integer; 0 for a key
    the dictionary does not hold — the reference would raise there, and its own query only measures entries behind a guard.  To every
    pass that walks expressions it is the field DISTINCT_FIELD of the looked-up entry."""
    def __init__(self, lookup):
        PayloadField.__init__(self, lookup, DISTINCT_FIELD)

    def __repr__(self):
        return "dictSize(%s[%r])" % (self.lookup.dict_name, self.lookup.key)


class RunNew(Expr):
    """Condition made by the EXECUTOR, never by the front end (engine.py: the fast route of a DistinctOp): this row is the first
    of its run of equal `key` values that carries `value`, among the rows passing `conds` (SDQH_X_RUNNEW, include/sdqh.h)."""
    def __init__(self, key, value, conds):
        self.key, self.value, self.conds = key, value, conds

    def __repr__(self):
        return "RunNew(%r, %r, %r)" % (self.key, self.value, self.conds)


class Lookup(Expr):
    """`tbl[key]`: key is an Expr or a RecordCons."""
    def __init__(self, dict_name, key):
        self.dict_name, self.key = dict_name, key

    def __repr__(self):
        return "Lookup(%s, %r)" % (self.dict_name, self.key)


class Const(Expr):
    def __init__(self, value):
        self.value = value

    def shape(self, names):
        return repr(self.value)

    def __repr__(self):
        return "Const(%r)" % (self.value,)


class Bin(Expr):
    def __init__(self, op, left, right):
        self.op, self.left, self.right = op, left, right

    def shape(self, names):
        return "(%s%s%s)" % (self.left.shape(names), self.op, self.right.shape(names))

    def __repr__(self):
        return "(%r %s %r)" % (self.left, self.op, self.right)


class Cmp(Expr):
    def __init__(self, op, left, right):
        self.op, self.left, self.right = op, left, right

    def __repr__(self):
        return "(%r %s %r)" % (self.left, self.op, self.right)


class And(Expr):
    def __init__(self, terms):
        self.terms = terms

    def __repr__(self):
        return "And(%s)" % ", ".join(map(repr, self.terms))


class Or(Expr):
    def __init__(self, terms):
        self.terms = terms

    def __repr__(self):
        return "Or(%s)" % ", ".join(map(repr, self.terms))


class Not(Expr):
    def __init__(self, term):
        self.term = term

    def __repr__(self):
        return "Not(%r)" % (self.term,)


class IfElse(Expr):
    """`a if cond else b` inside a value (reference IfExpr, lib/sdql_ir.py:294-303)."""
    def __init__(self, cond, then, other):
        self.cond, self.then, self.other = cond, then, other

    def shape(self, names):
        raise NotImplementedError           # not in the closed tuple vocabulary: goes through a row program

    def __repr__(self):
        return "(%r if %r else %r)" % (self.then, self.cond, self.other)


class Contains(Expr):
    """`tbl[key] != None` — the lookup must hit."""
    def __init__(self, lookup):
        self.lookup = lookup

    def __repr__(self):
        return "Contains(%r)" % self.lookup


class StrIn(Expr):
    """`"needle" in p[0].col` (how = "in"), `startsWith(p[0].col, "needle")` ("prefix"),
    `endsWith(p[0].col, "needle")` ("suffix")."""
    def __init__(self, needle, col, how="in"):
        self.needle, self.col, self.how = needle, col, how

    def __repr__(self):
        return "StrIn(%r %s %r)" % (self.needle, self.how, self.col)


class Call(Expr):
    def __init__(self, fn, args):
        self.fn, self.args = fn, args

    def shape(self, names):
        return "%s(%s)" % (self.fn, ",".join(a.shape(names) for a in self.args))

    def __repr__(self):
        return "%s(%s)" % (self.fn, ", ".join(map(repr, self.args)))


class RecordCons(Expr):
    def __init__(self, fields):
        self.fields = fields          # list of (name, Expr)

    def __repr__(self):
        return "record(%s)" % ", ".join("%s=%r" % f for f in self.fields)


class WholeKey(Expr):
    """`p[0]` / `p[1]` of a sum over a result dictionary; with `field`, `p[0].field` / `p[1].field`."""
    def __init__(self, which, field=None):
        self.which, self.field = which, field            # which: 0 = key, 1 = value

    def __repr__(self):
        return "kv[%d]%s" % (self.which, "" if self.field is None else "." + self.field)


class ConcatKV(Expr):
    """`p[0].concat(p[1])`."""

    def __repr__(self):
        return "kv[0].concat(kv[1])"


TRUE = Const(True)


# ---- operator IR --------------------------------------------------------------------------------
class ScanOp:
    """One loop over a database table."""
    def __init__(self, out, table, lineno):
        self.out, self.table, self.lineno = out, table, lineno
        self.conds = []         # conjunction of Cmp / Contains / StrIn
        self.kind = None        # "scalar" | "scalar_record" | "dict"
        self.fields = None      # scalar_record: [(name, Expr, [extra cond terms of that field])]
        self.key = None         # Expr | RecordCons                  (dict)
        self.val = None         # Expr | RecordCons | TRUE           (dict) / Expr (scalar)
        self.unique = False     # assignment sum: first insert wins, no aggregation
        self.dense = None       # dense(N, ...) size hint (ignored: sized from data)
        self.probe = None       # Lookup for joinProbe's index (must hit)

    def __repr__(self):
        return "ScanOp(%s <- %s%s: if %r: {%r: %r}%s)" % (self.out, self.table, " probe " + repr(self.probe) if self.probe else "",
                                                          self.conds, self.key, self.val, " unique" if self.unique else "")


class DistinctOp:
    """`T.sum(lambda p: {K: vector({V})} [if C else None])` over a database table: per key the SET of its values (the reference's
    K-E shape, generator_par.py's vector-valued dictionaries, as its Python mode evaluates them).  The only thing a later loop can do
    with the result is measure an entry: `dictSize(out[k])` (DistinctCount)."""
    def __init__(self, out, table, key, value, conds, lineno):
        self.out, self.table, self.key, self.value, self.conds, self.lineno = out, table, key, value, conds, lineno

    def __repr__(self):
        return "DistinctOp(%s <- %s: if %r: {%r: vector({%r})})" % (self.out, self.table, self.conds, self.key, self.value)


EXTREMA = {"smin": "min", "smax": "max"}
EXTREMA_WHERE = ("smin / smax are only supported as the whole value of a sum's dictionary, {key: smin(v)}, as a field of its record value, "
                 "{key: record({\"lo\": smin(v), ...})}, or as the whole body of a scalar sum, T.sum(lambda p: smax(v) [if c else None]) "
                 "- over a database table or a result dictionary, never in a condition, a key, arithmetic, another smin / smax, or a unique / join build")


class ExtremaOp:
    """`S.sum(lambda p: {K: smin(V)} ...)`, `{K: record({"lo": smin(V1), "hi": smax(V2), "total": W})}` or the scalar `smax(V)`, each
    possibly `if C else None`, over a database table (source_is_table) or a result dictionary: MIN / MAX aggregation, an extension
    of the language (the reference has sums only).  fields: [(name | None, "min" | "max" | None, Expr)] - None: an ordinary sum that
    shares the loop; key None: a scalar, read by later loops as any scalar sum (ScalarField).  NaN values are skipped; a key whose
    values were all NaN, or a scalar over no row, is NaN."""
    def __init__(self, out, source, source_is_table, key, fields, val_is_record, conds, lineno):
        self.out, self.source, self.source_is_table, self.key, self.fields = out, source, source_is_table, key, fields
        self.val_is_record, self.conds, self.lineno = val_is_record, conds, lineno
        self.table = source if source_is_table else None         # (Plan.fingerprint numbers the table parameters by this)

    def __repr__(self):
        def f(nm, how, e):
            body = "%s(%r)" % ("s" + how, e) if how else repr(e)
            return body if nm is None else "%s=%s" % (nm, body)
        val = ", ".join(f(*x) for x in self.fields)
        if self.val_is_record:
            val = "record(%s)" % val
        return "ExtremaOp(%s <- %s: if %r: %s)" % (self.out, self.source, self.conds, val if self.key is None else "{%r: %s}" % (self.key, val))


class ScalarField(Expr):
    """`name.field` of an earlier scalar-record sum (or `name` itself for a plain scalar sum)."""
    def __init__(self, name, field):
        self.name, self.field = name, field

    def __repr__(self):
        return "ScalarField(%s.%s)" % (self.name, self.field)


class ScalarExprOp:
    """Arithmetic over earlier scalar results, e.g. `(100.0 * li_probed.A) / li_probed.B` (Q14)."""
    def __init__(self, out, expr, lineno):
        self.out, self.expr, self.lineno = out, expr, lineno

    def __repr__(self):
        return "ScalarExprOp(%s = %r)" % (self.out, self.expr)


class SelectKeysOp:
    """HAVING: `{unique(p[0]): True} if p[1] <op> <const> else None` over an aggregated dictionary
    (Q18 `li_filtered`, test/test_all.py:879-885) — the keys whose value passes, as a set."""
    def __init__(self, out, source, conds, lineno):
        self.out, self.source, self.conds, self.lineno = out, source, conds, lineno

    def __repr__(self):
        return "SelectKeysOp(%s <- keys of %s where %r)" % (self.out, self.source, self.conds)


class HostDictOp:
    """A sum over a RESULT dictionary that is more than a reshape: conditions on its values, lookups
    into other results, arithmetic on its fields (reference K-F, generator 520-568, with lookups 85-96).
    O(groups), not O(rows): evaluated on the host over the materialised dictionaries."""
    def __init__(self, out, source, conds, key, val, unique, lineno):
        self.out, self.source, self.conds, self.key, self.val, self.unique, self.lineno = out, source, conds, key, val, unique, lineno

    def __repr__(self):
        return "HostDictOp(%s <- %s: if %r: {%r: %r})" % (self.out, self.source, self.conds, self.key, self.val)


class WrapScalarOp:
    """`sr_dict({record({"name": scalar}): True})`: a scalar result presented as a one-row result set (Q19)."""
    def __init__(self, out, fields, lineno):
        self.out, self.fields, self.lineno = out, fields, lineno          # [(name, Expr over earlier scalars)]

    def __repr__(self):
        return "WrapScalarOp(%s = %r)" % (self.out, self.fields)


class FinalizeOp:
    """Sum over a result dictionary that only reshapes (key, value) into one record set (K-F)."""
    def __init__(self, out, source, fields, lineno):
        self.out, self.source, self.fields, self.lineno = out, source, fields, lineno   # fields: None = concat, else [(name, 0 | 1[, field of that side])]


class Plan:
    def __init__(self, name, params, ops, result, consts):
        self.name, self.params, self.ops, self.result, self.consts = name, params, ops, result, consts

    def __repr__(self):
        return "Plan(%s(%s)):\n  " % (self.name, ", ".join(self.params)) + "\n  ".join(map(repr, self.ops)) + "\n  return " + str(self.result)

    def fingerprint(self):
        """The plan with every user-chosen name removed: table parameters become T0, T1, ... in order of
        first use, intermediate results D0, D1, ... in order of definition, and the terms of a
        conjunction are sorted.  Two formulations of one query that lower to the same loops have the
        same fingerprint whatever they call things (tests/golden/make_lowering_fixture.py)."""
        import re
        tables, dicts = [], [op.out for op in self.ops]
        for op in self.ops:
            t = getattr(op, "table", None)
            if t in self.params and t not in tables:
                tables.append(t)
        def canon(text):
            for i, n in enumerate(dicts):                       # (a record FIELD that happens to be called like a table or a result — `nation=` — is not one)
                text = re.sub(r"(?<![\w.])%s(?![\w=])" % re.escape(n), "D%d" % i, text)
            for i, n in enumerate(tables):
                text = re.sub(r"(?<![\w.])%s(?![\w=])" % re.escape(n), "T%d" % i, text)
            return text
        # two spellings that are one loop: a build whose value is its own key and whose entries nobody reads a field of
        # (`T.joinBuild("k", f, [])`, reference lib/sdql_ir.py:428-429) is the membership build `{unique(k): True}`; and the field
        # NAMES of a record used as a lookup key are not part of the loop (keys match by position: the reference's own q5 probes a
        # (s_suppkey, s_nationkey) dictionary with a (l_suppkey, c_nationkey) record)
        read_fields = set(re.findall(r"Payload\((\w+)\[", "\n".join(repr(op) for op in self.ops)))

        def val_of(op):
            if op.kind == "dict" and op.unique and isinstance(op.key, Col) and isinstance(op.val, RecordCons) and len(op.val.fields) == 1 \
                    and isinstance(op.val.fields[0][1], Col) and op.val.fields[0][1].name == op.key.name and op.out not in read_fields:
                return "Const(True)"
            return canon(repr(op.val))

        def anon_lookup_keys(text):
            def strip(m):
                return "Lookup(%s, record(%s" % (m.group(1), re.sub(r"(?<![\w.])\w+=", "", m.group(2)))
            prev = None
            while prev != text:
                prev = text
                text = re.sub(r"Lookup\((\w+), record\(([^()]*(?:\([^()]*(?:\([^()]*\))*[^()]*\))*[^()]*)", strip, text)
            return text
        def fin_fields(op):
            # K-F spelled `p[0].concat(p[1])` (fields None) and K-F spelled as the record of every key field, then every value field,
            # each under its own name, are one loop (the reference's q1 concatenates, test/test_all.py:62)
            if op.fields is None:
                return None
            src = next((o for o in self.ops if isinstance(o, ScanOp) and o.out == op.source), None)
            if src is not None and isinstance(src.key, RecordCons) and isinstance(src.val, RecordCons):
                whole = [(n, 0, n) for n, _ in src.key.fields] + [(n, 1, n) for n, _ in src.val.fields]
                if [tuple(f) for f in op.fields] == whole:
                    return None
            return op.fields
        lines = []
        for op in self.ops:
            if isinstance(op, ScanOp):
                conds = sorted(anon_lookup_keys(canon(repr(c))) for c in op.conds)
                fields = [(n, canon(repr(e)), sorted(canon(repr(c)) for c in fc)) for n, e, fc in (op.fields or [])]
                lines.append("scan %s <- %s probe=%s kind=%s unique=%s conds=%s key=%s val=%s fields=%s" % (
                    canon(op.out), canon(op.table), anon_lookup_keys(canon(repr(op.probe))), op.kind, op.unique, conds,
                    anon_lookup_keys(canon(repr(op.key))), anon_lookup_keys(val_of(op)), fields))
            elif isinstance(op, FinalizeOp):
                lines.append("finalize %s <- %s fields=%r" % (canon(op.out), canon(op.source), fin_fields(op)))
            elif isinstance(op, SelectKeysOp):
                lines.append("select %s <- %s where %s" % (canon(op.out), canon(op.source), sorted(canon(repr(c)) for c in op.conds)))
            elif isinstance(op, ScalarExprOp):
                lines.append("scalar %s = %s" % (canon(op.out), canon(repr(op.expr))))
            else:
                lines.append(canon(repr(op)))
        lines.append("return " + canon(self.result))
        return "\n".join(lines)


# ---- lowering -----------------------------------------------------------------------------------
_BINOPS = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*", ast.Div: "/"}
_CMPOPS = {ast.Lt: "<", ast.LtE: "<=", ast.Gt: ">", ast.GtE: ">=", ast.Eq: "==", ast.NotEq: "!="}



# =================================================================================================
# Nested dictionaries (the reference's K-G, sdql_ir_cpp_generator_par.py:530-534, 757-760) and sums of a record of a scalar and a
# dictionary have no loop shape of their own here; the reference's own TPCH script uses them in three queries (test/test_all.py: q11
# 562-604, q12 608-652, q16 760-827).  They are rewritten, statement by statement, into the flat forms the planner has kernels for —
# the same rewrites sdqlpy_amd/tpch_queries.py applies by hand:
#
#   X = T.joinProbe(i, c, f, lambda e, r: record({"A": a, "B": sr_dict({k: v})}))      one loop per field:  X__A = ... a,  X__B = ... {k: v};
#                                                                                     `X.A` / `X.B` later name those results
#   L = T.sum(lambda p: {K1: sr_dict({K2: V})} if c else None)                         L keyed by the record (K1, K2)
#   O = U.joinProbe(L, col, f, lambda e, r: e.sum(lambda q: BODY))                     the join turned round: U indexed on col, then a sum over
#                                                                                     L's entries that looks the U row up (BODY's q[0] is the
#                                                                                     entry's K2, r.x the looked-up row's x)
#   P = U.joinProbe(i, c, f, lambda e, r: {K: sr_dict({K2: True})} if c else None)     P = the distinct (K fields, K2) combinations
#   R = P.sum(lambda p: {p[0].concat(record({"n": dictSize(p[1])})): True})            their number per K, then the usual reshape
# =================================================================================================
_NEST_OUTER, _NEST_INNER = "nest_outer", "nest_inner"


def _strip_conds(node):
    """BODY if C1 else None ... -> (BODY, [C tests, outermost first])"""
    tests = []
    while isinstance(node, ast.IfExp):
        tests.append((node.test, node.orelse))
        node = node.body
    return node, tests


def _wrap_conds(body, tests):
    for test, orelse in reversed(tests):
        body = ast.IfExp(test=test, body=body, orelse=orelse)
    return body


def _inner_dict(node):
    """sr_dict({k: v}) or {k: v} -> (k, v), else None"""
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "sr_dict" and len(node.args) == 1:
        node = node.args[0]
    if isinstance(node, ast.Dict) and len(node.keys) == 1:
        return node.keys[0], node.values[0]
    return None


def _record_fields(node):
    """record({"a": x, ...}) -> [(name, node)], else None"""
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "record" and len(node.args) == 1 \
            and isinstance(node.args[0], ast.Dict) and all(isinstance(k, ast.Constant) and isinstance(k.value, str) for k in node.args[0].keys):
        return [(k.value, v) for k, v in zip(node.args[0].keys, node.args[0].values)]
    return None


def _record_node(fields):
    return ast.Call(func=ast.Name(id="record", ctx=ast.Load()), args=[ast.Dict(keys=[ast.Constant(value=n) for n, _ in fields], values=[v for _, v in fields])], keywords=[])


class _Subst(ast.NodeTransformer):
    def __init__(self, fn):
        self.fn = fn

    def visit(self, node):
        new = self.fn(node)
        if new is not None:
            return new
        return self.generic_visit(node)


def _subst(node, fn):
    import copy
    return ast.fix_missing_locations(_Subst(fn).visit(copy.deepcopy(node)))


def _table_call(val):
    """X = T.method(...) with a lambda as output function -> (table name, method, args, index of the output lambda), else None"""
    if not (isinstance(val, ast.Call) and isinstance(val.func, ast.Attribute) and isinstance(val.func.value, ast.Name)):
        return None
    m = val.func.attr
    if m == "sum" and val.args and isinstance(val.args[0], ast.Lambda):
        return val.func.value.id, m, val.args, 0
    if m == "joinProbe" and len(val.args) >= 4 and isinstance(val.args[3], ast.Lambda):
        return val.func.value.id, m, val.args, 3
    return None


def _with_body(val, idx, body):
    import copy
    new = copy.deepcopy(val)
    new.args[idx].body = body
    return new


def _desugar(fdef):
    """The function's statements with the nested forms above rewritten (a new list; the input is not modified)."""
    import copy
    params = {a.arg for a in fdef.args.args}
    split = {}          # X -> {field: flat name}
    nested = {}         # L -> True: keyed by record(nest_outer, nest_inner)
    nested_set = {}     # P -> [field names of K] (plus nest_inner)
    out = []

    def rename(node):   # X.F -> X__F for split results
        def fn(n):
            if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id in split and n.attr in split[n.value.id]:
                return ast.copy_location(ast.Name(id=split[n.value.id][n.attr], ctx=ast.Load()), n)
            return None
        return _subst(node, fn)

    for st in fdef.body:
        st = rename(st) if split else st
        if not (isinstance(st, ast.Assign) and len(st.targets) == 1 and isinstance(st.targets[0], ast.Name)):
            out.append(st)
            continue
        name, val = st.targets[0].id, st.value
        tc = _table_call(val)
        if tc is None:
            out.append(st)
            continue
        table, method, args, li = tc
        lam = args[li]
        body, tests = _strip_conds(lam.body)

        def assign(target, value, like=st):
            return ast.fix_missing_locations(ast.copy_location(ast.Assign(targets=[ast.Name(id=target, ctx=ast.Store())], value=value), like))

        # ---- a record of sums, at least one of them a dictionary: one loop per field ----
        fields = _record_fields(body)
        if fields is not None and any(_inner_dict(v) is not None for _, v in fields) and table not in nested and table not in nested_set:
            split[name] = {}
            for fname, v in fields:
                inner = _inner_dict(v)
                fbody = ast.Dict(keys=[inner[0]], values=[inner[1]]) if inner is not None else v
                flat = "%s__%s" % (name, fname)
                split[name][fname] = flat
                out.append(assign(flat, _with_body(val, li, _wrap_conds(fbody, tests))))
            continue
        # ---- the outer loop of a nested dictionary: {K1: sr_dict({K2: V})} ----
        if isinstance(body, ast.Dict) and len(body.keys) == 1 and _inner_dict(body.values[0]) is not None and not isinstance(body.values[0], ast.Dict) or \
                (isinstance(body, ast.Dict) and len(body.keys) == 1 and isinstance(body.values[0], ast.Dict) and len(body.values[0].keys) == 1):
            k1 = body.keys[0]
            k2, v = _inner_dict(body.values[0])
            if isinstance(v, ast.Constant) and v.value is True:
                kf = _record_fields(k1) or [(_NEST_OUTER, k1)]
                nested_set[name] = [n for n, _ in kf]
                new_body = ast.Dict(keys=[_record_node(kf + [(_NEST_INNER, k2)])], values=[ast.Constant(value=1)])
            else:
                nested[name] = True
                new_body = ast.Dict(keys=[_record_node([(_NEST_OUTER, k1), (_NEST_INNER, k2)])], values=[v])
            out.append(assign(name, _with_body(val, li, _wrap_conds(new_body, tests))))
            continue
        # ---- a probe whose output function sums over the matched inner dictionary ----
        if method == "joinProbe" and isinstance(args[0], ast.Name) and args[0].id in nested and isinstance(body, ast.Call) \
                and isinstance(body.func, ast.Attribute) and body.func.attr == "sum" and isinstance(body.func.value, ast.Name) \
                and body.func.value.id == lam.args.args[0].arg and body.args and isinstance(body.args[0], ast.Lambda) and not tests:
            src = args[0].id
            row = lam.args.args[1].arg                          # the probing row's name in the output function
            inner_lam = body.args[0]
            q = inner_lam.args.args[0].arg
            idx = "%s__index" % name
            used = []
            for n in ast.walk(inner_lam.body):
                if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == row and n.attr not in used:
                    used.append(n.attr)
            colname = args[1]
            outcols = ast.List(elts=[ast.Constant(value=c) for c in used] or [copy.deepcopy(colname)], ctx=ast.Load())
            build = ast.Call(func=ast.Attribute(value=ast.Name(id=table, ctx=ast.Load()), attr="joinBuild", ctx=ast.Load()),
                             args=[copy.deepcopy(colname), copy.deepcopy(args[2]), outcols], keywords=[])
            out.append(assign(idx, build))

            def entry_key(which):                               # q[0].nest_outer / q[0].nest_inner
                return ast.Attribute(value=ast.Subscript(value=ast.Name(id=q, ctx=ast.Load()), slice=ast.Constant(value=0), ctx=ast.Load()), attr=which, ctx=ast.Load())

            def looked_up():
                return ast.Subscript(value=ast.Name(id=idx, ctx=ast.Load()), slice=entry_key(_NEST_OUTER), ctx=ast.Load())

            def fn(n):
                if isinstance(n, ast.Subscript) and isinstance(n.value, ast.Name) and n.value.id == q:
                    i = n.slice.value if isinstance(n.slice, ast.Constant) else getattr(getattr(n.slice, "value", None), "value", None)
                    if i == 0:
                        return entry_key(_NEST_INNER)
                    return n
                if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == row:
                    return ast.Attribute(value=looked_up(), attr=n.attr, ctx=ast.Load())
                return None
            new_inner = _subst(inner_lam.body, fn)
            found = ast.Compare(left=looked_up(), ops=[ast.NotEq()], comparators=[ast.Constant(value=None)])
            new_lam = ast.Lambda(args=copy.deepcopy(inner_lam.args), body=ast.IfExp(test=found, body=new_inner, orelse=ast.Constant(value=None)))
            call = ast.Call(func=ast.Attribute(value=ast.Name(id=src, ctx=ast.Load()), attr="sum", ctx=ast.Load()), args=[new_lam], keywords=[])
            out.append(assign(name, call))
            continue
        # ---- the size of the inner set per outer key ----
        if method == "sum" and table in nested_set and isinstance(body, ast.Dict) and len(body.keys) == 1 and not tests:
            key = body.keys[0]
            p = lam.args.args[0].arg
            if isinstance(key, ast.Call) and isinstance(key.func, ast.Attribute) and key.func.attr == "concat" and len(key.args) == 1:
                cf = _record_fields(key.args[0])
                sizes = cf is not None and all(isinstance(v, ast.Call) and isinstance(v.func, ast.Name) and v.func.id == "dictSize" for _, v in cf)
                if sizes:
                    def pkey(f):
                        return ast.Attribute(value=ast.Subscript(value=ast.Name(id=p, ctx=ast.Load()), slice=ast.Constant(value=0), ctx=ast.Load()), attr=f, ctx=ast.Load())
                    cnt = "%s__sizes" % table
                    grp = ast.Dict(keys=[_record_node([(f, pkey(f)) for f in nested_set[table]])], values=[_record_node([(n, ast.Constant(value=1)) for n, _ in cf])])
                    out.append(assign(cnt, ast.Call(func=ast.Attribute(value=ast.Name(id=table, ctx=ast.Load()), attr="sum", ctx=ast.Load()),
                                                    args=[ast.Lambda(args=copy.deepcopy(lam.args), body=grp)], keywords=[])))
                    whole = ast.Call(func=ast.Attribute(value=ast.Subscript(value=ast.Name(id=p, ctx=ast.Load()), slice=ast.Constant(value=0), ctx=ast.Load()), attr="concat", ctx=ast.Load()),
                                     args=[ast.Subscript(value=ast.Name(id=p, ctx=ast.Load()), slice=ast.Constant(value=1), ctx=ast.Load())], keywords=[])
                    out.append(assign(name, ast.Call(func=ast.Attribute(value=ast.Name(id=cnt, ctx=ast.Load()), attr="sum", ctx=ast.Load()),
                                                     args=[ast.Lambda(args=copy.deepcopy(lam.args), body=ast.Dict(keys=[whole], values=[body.values[0]]))], keywords=[])))
                    continue
        # ---- a table loop that yields a set of wide records: {unique(record({...looked-up / text fields...})): True} ----
        # (the reference's q2, test/test_all.py:119-139): the rows that pass, identified by the scanned row's own columns the record
        # is a function of, then the record per such row — the author's unique() says distinct rows give distinct records
        if method == "sum" and table in params and isinstance(body, ast.Dict) and len(body.keys) == 1 \
                and isinstance(body.values[0], ast.Constant) and body.values[0].value is True \
                and isinstance(body.keys[0], ast.Call) and isinstance(body.keys[0].func, ast.Name) and body.keys[0].func.id == "unique" and len(body.keys[0].args) == 1:
            fields = _record_fields(body.keys[0].args[0])
            p = lam.args.args[0].arg

            def row_cols(node):
                found = []
                for n in ast.walk(node):
                    if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Subscript) and isinstance(n.value.value, ast.Name) and n.value.value.id == p \
                            and isinstance(n.value.slice, ast.Constant) and n.value.slice.value == 0 and n.attr not in found:
                        found.append(n.attr)
                return found

            def plain(node):
                return isinstance(node, ast.Attribute) and row_cols(node) == [node.attr] and isinstance(node.value, ast.Subscript)
            if fields is not None and len(fields) > 2 and not all(plain(v) for _, v in fields):
                cols = row_cols(body.keys[0].args[0])
                if 1 <= len(cols) <= 2:
                    rows = "%s__rows" % name
                    pick = ast.Dict(keys=[_record_node([(c, ast.Attribute(value=ast.Subscript(value=ast.Name(id=p, ctx=ast.Load()), slice=ast.Constant(value=0), ctx=ast.Load()),
                                                                          attr=c, ctx=ast.Load())) for c in cols])], values=[ast.Constant(value=1)])
                    out.append(assign(rows, _with_body(val, li, _wrap_conds(pick, tests))))
                    # (p[0].c of the entry IS the scanned row's c: the record's expression carries over as it stands)
                    call = ast.Call(func=ast.Attribute(value=ast.Name(id=rows, ctx=ast.Load()), attr="sum", ctx=ast.Load()),
                                    args=[ast.Lambda(args=copy.deepcopy(lam.args), body=copy.deepcopy(body))], keywords=[])
                    out.append(assign(name, call))
                    continue
        out.append(st)
    return out


class _Lowerer:
    def __init__(self, fn_name, source_lines, first_line, outer_consts=None):
        self.fn_name, self.lines, self.first_line = fn_name, source_lines, first_line
        self.consts = dict(outer_consts or {})      # numbers / text bound outside the function (closure, module) + local literals
        self.scalars = set()     # names bound to scalar / scalar-record sums
        self.params = []
        self.dicts = set()      # names bound to operator outputs
        self.vectors = set()    # ... those that are dictionaries of sets (DistinctOp): only dictSize(name[key]) may read them

    def fail(self, node, why):
        ln = getattr(node, "lineno", 0)
        text = self.lines[ln - 1].strip() if 0 < ln <= len(self.lines) else ""
        raise UnsupportedQuery("%s, line %d: %s\n    %s" % (self.fn_name, self.first_line + ln - 1, why, text))

    # -- expressions ------------------------------------------------------------------------
    def expr(self, node, env):
        """env: {python name: ("row",) | ("payload", Lookup) | ("kv",)}"""
        if isinstance(node, ast.Constant):
            return Const(node.value)
        if isinstance(node, ast.Name):
            if node.id in self.consts:
                return Const(self.consts[node.id])
            if node.id in env and env[node.id][0] == "payload":
                return PayloadField(env[node.id][1], None)
            if node.id in self.scalars:
                return ScalarField(node.id, None)
            self.fail(node, "unknown name '%s'" % node.id)
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub) and isinstance(node.operand, ast.Constant):
            return Const(-node.operand.value)
        if isinstance(node, ast.Attribute):
            base = node.value
            # p[0].x
            if isinstance(base, ast.Subscript) and isinstance(base.value, ast.Name) and env.get(base.value.id, (None,))[0] in ("rowpair", "kv"):
                idx = self._index(base)
                kind = env[base.value.id][0]
                if kind == "rowpair" and idx == 0:
                    return Col(node.attr)
                if kind == "kv":
                    return WholeKey(idx, node.attr)
                self.fail(node, "only p[0].<column> is supported inside a table sum")
            if isinstance(base, ast.Name) and base.id in self.scalars and base.id not in env:
                return ScalarField(base.id, node.attr)
            if isinstance(base, ast.Name) and base.id in env:
                kind = env[base.id]
                if kind[0] == "row":
                    return Col(node.attr)
                if kind[0] == "payload":
                    return PayloadField(kind[1], node.attr)
            inner = self.expr(base, env)
            if isinstance(inner, Lookup):
                return PayloadField(inner, node.attr)
            self.fail(node, "unsupported attribute access")
        if isinstance(node, ast.Subscript):
            if isinstance(node.value, ast.Name) and node.value.id in self.vectors:
                self.fail(node, "an entry of '%s' is a set: only its size can be read, dictSize(%s[key])" % (node.value.id, node.value.id))
            if isinstance(node.value, ast.Name) and node.value.id in self.dicts:
                key = self.expr(self._slice(node), env)
                return Lookup(node.value.id, key)
            if isinstance(node.value, ast.Name) and env.get(node.value.id, (None,))[0] == "kv":
                return WholeKey(self._index(node))
            self.fail(node, "unsupported subscript")
        if isinstance(node, ast.BinOp) and type(node.op) in _BINOPS:
            left, right = self.expr(node.left, env), self.expr(node.right, env)
            if isinstance(node.op, ast.Mult) and self._is_bool(left) and self._is_bool(right):
                return And(self._terms(left) + self._terms(right))    # `a * b` on booleans is AND (ref sdql_compiler.py:277-292)
            return Bin(_BINOPS[type(node.op)], left, right)
        if isinstance(node, ast.BoolOp) and isinstance(node.op, ast.And):
            terms = []
            for v in node.values:
                terms += self._terms(self.expr(v, env))
            return And(terms)
        if isinstance(node, ast.BoolOp) and isinstance(node.op, ast.Or):           # reference prints `or` as `+` on 0/1 values (sdql_compiler.py:277-292)
            terms = []
            for v in node.values:
                t = self.expr(v, env)
                if not self._is_bool(t):
                    self.fail(v, "operand of `or` is not a condition")
                terms += t.terms if isinstance(t, Or) else [t]
            return Or(terms)
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.Not):
            t = self.expr(node.operand, env)
            if not self._is_bool(t):
                self.fail(node, "operand of `not` is not a condition")
            return t.term if isinstance(t, Not) else Not(t)
        if isinstance(node, ast.IfExp):                                          # a conditional VALUE: `x if c else y`
            cond = self.expr(node.test, env)
            if not self._is_bool(cond):
                self.fail(node.test, "condition is not a comparison")
            return IfElse(cond, self.expr(node.body, env), self.expr(node.orelse, env))
        if isinstance(node, ast.Compare) and len(node.ops) > 1:
            # chained comparison `a <= x < b`: the conjunction of its links (Python evaluates it that way)
            terms, left = [], node.left
            for op, right in zip(node.ops, node.comparators):
                link = ast.copy_location(ast.Compare(left=left, ops=[op], comparators=[right]), node)
                terms += self._terms(self.expr(link, env))
                left = right
            return And(terms)
        if isinstance(node, ast.Compare) and len(node.ops) == 1:
            op = node.ops[0]
            left, right = self.expr(node.left, env), self.expr(node.comparators[0], env)
            if isinstance(op, ast.In):
                if isinstance(left, Const) and isinstance(left.value, str) and isinstance(right, Col):
                    return StrIn(left.value, right)
                self.fail(node, "`in` is only supported as \"text\" in <string column>")
            if type(op) not in _CMPOPS:
                self.fail(node, "unsupported comparison")
            sym = _CMPOPS[type(op)]
            if isinstance(right, Const) and right.value is None and sym in ("!=", "=="):      # `tbl[k] != None` / `== None`
                lk = left if isinstance(left, Lookup) else (left.lookup if isinstance(left, PayloadField) and left.field is None else None)
                if lk is None:
                    self.fail(node, "only a dictionary lookup can be compared with None")
                return Contains(lk) if sym == "!=" else Not(Contains(lk))
            if isinstance(right, Const) and isinstance(right.value, bool) and self._is_bool(left) and sym in ("==", "!="):   # `(cond) == False`
                return left if (right.value is True) == (sym == "==") else Not(left)
            if isinstance(left, Const) and not isinstance(right, Const):          # constant on the right: `5 <= x` is `x >= 5`
                left, right, sym = right, left, {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "==": "==", "!=": "!="}[sym]
            return Cmp(sym, left, right)
        if isinstance(node, ast.Call):
            fn = node.func
            if isinstance(fn, ast.Name):
                if fn.id == "record" and len(node.args) == 1 and isinstance(node.args[0], ast.Dict):
                    d = node.args[0]
                    fields = []
                    for k, v in zip(d.keys, d.values):
                        if not (isinstance(k, ast.Constant) and isinstance(k.value, str)):
                            self.fail(node, "record field names must be string literals")
                        fields.append((k.value, self.expr(v, env)))
                    return RecordCons(fields)
                if fn.id == "unique" and len(node.args) == 1:
                    return Call("unique", [self.expr(node.args[0], env)])
                if fn.id == "dense" and len(node.args) == 2:
                    return Call("dense", [self.expr(node.args[0], env), self.expr(node.args[1], env)])
                if fn.id == "extractYear" and len(node.args) == 1:
                    return Call("extractYear", [self.expr(node.args[0], env)])
                if fn.id in ("startsWith", "endsWith") and len(node.args) == 2:       # ref sdql_lib.py:347-351
                    col, needle = self.expr(node.args[0], env), self.expr(node.args[1], env)
                    if isinstance(col, Col) and isinstance(needle, Const) and isinstance(needle.value, str):
                        return StrIn(needle.value, col, "prefix" if fn.id == "startsWith" else "suffix")
                    self.fail(node, "%s needs (<string column>, \"text\")" % fn.id)
                if fn.id == "firstIndex" and len(node.args) == 2:                       # ref sdql_lib.py:344-345, include/varchar.h:91-97
                    col, needle = self.expr(node.args[0], env), self.expr(node.args[1], env)
                    if isinstance(col, Col) and isinstance(needle, Const) and isinstance(needle.value, str):
                        return Call("firstIndex", [col, needle])
                    self.fail(node, "firstIndex needs (<string column>, \"text\")")
                if fn.id == "substr" and len(node.args) == 3:                           # ref sdql_lib.py:362-363: source[start:end + 1]
                    col, a, b = (self.expr(x, env) for x in node.args)
                    if isinstance(col, Col) and all(isinstance(x, Const) and isinstance(x.value, int) for x in (a, b)) and 0 <= a.value <= b.value:
                        return Call("substr", [col, a, b])
                    self.fail(node, "substr needs (<string column>, start, end) with literal bounds")
                if fn.id == "dictSize" and len(node.args) == 1:
                    arg = node.args[0]
                    if isinstance(arg, ast.Subscript) and isinstance(arg.value, ast.Name) and arg.value.id in self.vectors:
                        return DistinctCount(Lookup(arg.value.id, self.expr(self._slice(arg), env)))
                    self.fail(node, "dictSize is only supported as dictSize(tbl[key]) with tbl a dictionary of sets, T.sum(lambda p: {k: vector({v})})")
                if fn.id in EXTREMA:
                    self.fail(node, EXTREMA_WHERE)
                if fn.id == "vector":
                    self.fail(node, "vector({...}) is only supported as the whole value of a table sum's dictionary, {key: vector({value})}")
            if isinstance(fn, ast.Attribute) and fn.attr == "concat" and len(node.args) == 1:
                a, b = self.expr(fn.value, env), self.expr(node.args[0], env)
                if isinstance(a, WholeKey) and isinstance(b, WholeKey) and a.which == 0 and b.which == 1:
                    return ConcatKV()
            self.fail(node, "unsupported call")
        self.fail(node, "unsupported expression (%s)" % type(node).__name__)

    @staticmethod
    def _slice(node):
        s = node.slice
        return s.value if isinstance(s, ast.Index) else s        # py3.8 compatibility

    def _index(self, node):
        s = self._slice(node)
        if isinstance(s, ast.Constant) and s.value in (0, 1):
            return s.value
        self.fail(node, "expected [0] or [1]")

    @staticmethod
    def _is_bool(e):
        return isinstance(e, (Cmp, And, Or, Not, Contains, StrIn)) or (isinstance(e, Const) and isinstance(e.value, bool))

    @staticmethod
    def _terms(e):
        if isinstance(e, And):
            return list(e.terms)
        if isinstance(e, Const) and e.value is True:
            return []
        return [e]

    # -- lambda bodies ----------------------------------------------------------------------
    def split_ifelse(self, node, env):
        """`BODY if COND else <zero>` -> (BODY node, [cond terms]); plain BODY -> (BODY, [])."""
        conds = []
        while isinstance(node, ast.IfExp):
            orelse = node.orelse
            zero = (isinstance(orelse, ast.Constant) and orelse.value in (None, 0, 0.0)) or \
                   (isinstance(orelse, ast.Call) and isinstance(orelse.func, ast.Name) and orelse.func.id == "sr_dict" and not orelse.args)
            if not zero:
                self.fail(node, "the else arm of a conditional sum must be None / 0.0 / sr_dict()")
            cond = self.expr(node.test, env)
            if not self._is_bool(cond):
                self.fail(node.test, "condition is not a comparison")
            conds += self._terms(cond)
            node = node.body
        return node, conds

    @staticmethod
    def _is_dict_valued(node):
        while isinstance(node, ast.IfExp):
            node = node.body
        return isinstance(node, ast.Dict)

    def dict_body(self, op, node, env, vectors_ok=False):
        """{K: V}; with vectors_ok, V may be vector({E}): op.val = ("vector", E)"""
        if not (isinstance(node, ast.Dict) and len(node.keys) == 1):
            self.fail(node, "expected a one-entry dictionary {key: value}")
        key = self.expr(node.keys[0], env)
        while isinstance(key, Call) and key.fn in ("unique", "dense"):
            if key.fn == "unique":
                op.unique = True
                key = key.args[0]
            else:
                op.dense = key.args[0].value if isinstance(key.args[0], Const) else None
                key = key.args[1]
        op.key = key
        op.kind = "dict"
        v = node.values[0]
        if isinstance(v, ast.Call) and isinstance(v.func, ast.Name) and v.func.id == "vector":
            if not (vectors_ok and len(v.args) == 1 and isinstance(v.args[0], ast.Set) and len(v.args[0].elts) == 1):
                self.fail(v, "vector({...}) is only supported as the value of a sum over a database table, holding one expression: {key: vector({value})}")
            op.val = ("vector", self.expr(v.args[0].elts[0], env))
            return
        op.val = self.expr(v, env)

    # -- MIN / MAX ---------------------------------------------------------------------------
    @staticmethod
    def _extremum(node):
        """smin(V) / smax(V) -> ("min" | "max", V node), else None"""
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in EXTREMA and len(node.args) == 1 and not node.keywords:
            return EXTREMA[node.func.id], node.args[0]
        return None

    def extrema_op(self, out, source, is_table, body, conds, env, ln):
        """The ExtremaOp of a sum's body (conditions already split off) when smin / smax stands in one of its positions, else None
        (an smin / smax anywhere else is refused where the expression is lowered: expr)."""
        key, val_is_record = None, False
        if isinstance(body, ast.Dict) and len(body.keys) == 1:
            v = body.values[0]
            rec = _record_fields(v)
            if self._extremum(v) is not None:
                pairs = [(None, v)]
            elif rec is not None and any(self._extremum(x) is not None for _, x in rec):
                pairs, val_is_record = rec, True
            else:
                return None
            key = self.expr(body.keys[0], env)
            while isinstance(key, Call) and key.fn in ("unique", "dense"):
                if key.fn == "unique":
                    self.fail(body, "smin / smax under a unique() key: a first-row-wins build aggregates nothing")
                key = key.args[1]
        elif self._extremum(body) is not None:
            pairs = [(None, body)]
        else:
            return None
        fields = []
        for nm, x in pairs:
            how = self._extremum(x)
            fields.append((nm, how[0], self.expr(how[1], env)) if how is not None else (nm, None, self.expr(x, env)))
        if len(fields) > 4:                                          # SDQH_TUPLE_MAX_VALUES
            self.fail(body, "more than 4 values (extrema and sums together) in one loop")
        if key is None:
            self.scalars.add(out)
        return ExtremaOp(out, source, is_table, key, fields, val_is_record, conds, ln)

    # -- statements -------------------------------------------------------------------------
    def lambda_of(self, node, nparams):
        if not (isinstance(node, ast.Lambda) and len(node.args.args) == nparams):
            self.fail(node, "expected a lambda with %d parameter(s)" % nparams)
        return [a.arg for a in node.args.args], node.body

    def lower_call(self, out, call):
        fn = call.func
        table = fn.value.id
        ln = call.lineno
        if table in self.params:
            op = ScanOp(out, table, ln)
            if fn.attr == "sum":
                if not 1 <= len(call.args) <= 2:
                    self.fail(call, "sum takes (lambda[, is_update])")
                (p,), body = self.lambda_of(call.args[0], 1)
                env = {p: ("rowpair",)}
                body, conds = self.split_ifelse(body, env)
                op.conds = conds
                ext = self.extrema_op(out, table, True, body, conds, env, ln)
                if ext is not None:
                    if len(call.args) == 2 and isinstance(call.args[1], ast.Constant) and call.args[1].value is False:
                        self.fail(call, "smin / smax in an assignment sum (is_update False): a first-row-wins build aggregates nothing")
                    return ext
                if isinstance(body, ast.Dict):
                    self.dict_body(op, body, env, vectors_ok=True)
                    if isinstance(op.val, tuple):                     # {K: vector({V})}: per key the set of its values
                        if isinstance(op.key, RecordCons) or isinstance(op.val[1], RecordCons):
                            self.fail(body, "a dictionary of sets needs a single key and a single value expression")
                        return DistinctOp(out, table, op.key, op.val[1], conds, ln)
                elif isinstance(body, ast.Call) and isinstance(body.func, ast.Name) and body.func.id == "record" \
                        and len(body.args) == 1 and isinstance(body.args[0], ast.Dict):
                    # record of independent sums, each possibly under its own condition (Q14: test/test_all.py:703-711)
                    op.kind, op.fields = "scalar_record", []
                    for k, v in zip(body.args[0].keys, body.args[0].values):
                        if not (isinstance(k, ast.Constant) and isinstance(k.value, str)):
                            self.fail(body, "record field names must be string literals")
                        fbody, fconds = self.split_ifelse(v, env)
                        op.fields.append((k.value, self.expr(fbody, env), fconds))
                    self.scalars.add(out)
                else:
                    op.kind, op.val = "scalar", self.expr(body, env)
                    self.scalars.add(out)
                if len(call.args) == 2 and isinstance(call.args[1], ast.Constant) and call.args[1].value is False:
                    op.unique = True
                self._promote_probe(op)
                return op
            if fn.attr == "joinBuild":
                if len(call.args) != 3:
                    self.fail(call, "joinBuild takes (column, filter, outCols)")
                colname = self._const_str(call.args[0])
                (p,), body = self.lambda_of(call.args[1], 1)
                env = {p: ("rowpair",)}
                cond = self.expr(body, env)
                op.conds = self._terms(cond) if self._is_bool(cond) else self.fail(body, "filter is not a comparison")
                if not isinstance(call.args[2], ast.List):
                    self.fail(call, "outCols must be a list literal")
                outcols = [self._const_str(e) for e in call.args[2].elts]
                op.kind, op.unique = "dict", True
                op.key = Col(colname)
                # outCols == [] keeps the key itself as the value (ref lib/sdql_ir.py:428-429)
                op.val = RecordCons([(c, Col(c)) for c in (outcols or [colname])])
                return op
            if fn.attr == "joinProbe":
                if not 4 <= len(call.args) <= 5:
                    self.fail(call, "joinProbe takes (index, column, filter, outputFunc[, is_update])")
                if not (isinstance(call.args[0], ast.Name) and call.args[0].id in self.dicts):
                    self.fail(call, "joinProbe's index must be the result of an earlier build")
                if call.args[0].id in self.vectors:
                    self.fail(call, "'%s' is a dictionary of sets: it cannot be a joinProbe index (only dictSize(%s[key]) reads it)" % (call.args[0].id, call.args[0].id))
                colname = self._const_str(call.args[1])
                (p,), fbody = self.lambda_of(call.args[2], 1)
                cond = self.expr(fbody, {p: ("rowpair",)})
                op.conds = self._terms(cond) if self._is_bool(cond) else self.fail(fbody, "filter is not a comparison")
                op.probe = Lookup(call.args[0].id, Col(colname))
                (pv, pk), body = self.lambda_of(call.args[3], 2)
                env = {pv: ("payload", op.probe), pk: ("row",)}
                if not self._is_dict_valued(body):
                    # a scalar body: `joinProbe(idx, col, f, lambda e, r: x if c else 0.0)` sums x over the matching rows (Q17, Q19)
                    body, conds = self.split_ifelse(body, env)
                    op.conds += conds
                    op.kind, op.val = "scalar", self.expr(body, env)
                    self.scalars.add(out)
                    return op
                body, conds = self.split_ifelse(body, env)
                op.conds += conds
                self.dict_body(op, body, env)
                if len(call.args) == 5:
                    if not isinstance(call.args[4], ast.Constant):
                        self.fail(call, "is_update must be a literal")
                    if call.args[4].value is False:
                        op.unique = True        # 5th arg False => assignment sum (ref sdql_compiler.py:203-205)
                return op
            self.fail(call, "unsupported table method '%s'" % fn.attr)
        if table in self.vectors:
            self.fail(call, "'%s' is a dictionary of sets: it cannot be summed over (only dictSize(%s[key]) reads it)" % (table, table))
        if table in self.dicts and fn.attr == "sum":
            (p,), body = self.lambda_of(call.args[0], 1)
            env = {p: ("kv",)}
            tmp = ScanOp(out, table, ln)
            body, kv_conds = self.split_ifelse(body, env)
            ext = self.extrema_op(out, table, False, body, kv_conds, env, ln)
            if ext is not None:
                return ext
            if not isinstance(body, ast.Dict):
                self.fail(call, "a sum over a result dictionary must build a dictionary {key: value}")
            self.dict_body(tmp, body, env)
            set_valued = isinstance(tmp.val, Const) and tmp.val.value is True
            if kv_conds:
                simple = tmp.unique and set_valued and isinstance(tmp.key, WholeKey) and tmp.key.which == 0 and tmp.key.field is None \
                    and all(isinstance(c, Cmp) and isinstance(c.left, WholeKey) and c.left.which == 1 and c.left.field is None and isinstance(c.right, Const)
                            and isinstance(c.right.value, (int, float)) and c.op in ("<", "<=", ">", ">=", "==") for c in kv_conds)
                if simple:
                    return SelectKeysOp(out, table, kv_conds, ln)
            elif set_valued:                                        # the reference's own queries write the reshape without unique() at times (Q16)
                if isinstance(tmp.key, ConcatKV):
                    return FinalizeOp(out, table, None, ln)
                if isinstance(tmp.key, RecordCons) and all(isinstance(e, WholeKey) for _, e in tmp.key.fields):
                    return FinalizeOp(out, table, [(n, e.which) if e.field is None else (n, e.which, e.field) for n, e in tmp.key.fields], ln)
            # anything else over a result dictionary (HAVING with lookups, arithmetic on its fields): host-side, O(groups)
            return HostDictOp(out, table, kv_conds, tmp.key, tmp.val, tmp.unique, ln)
        self.fail(call, "'%s' is neither a table parameter nor an earlier result" % table)

    @staticmethod
    def _promote_probe(op):
        """`T.sum(lambda r: {K: V} if ... and idx[r[0].col] != None else None)` IS
        `T.joinProbe(idx, "col", ..., lambda entry, row: {K: V})` (reference lib/sdql_ir.py:443-454
        defines joinProbe as exactly that sum): give both spellings one IR.  The promoted lookup is the
        one whose entry the body reads fields of, else the first membership condition on a plain column."""
        if op.kind != "dict" or op.probe is not None:
            return
        cands = [c for c in op.conds if isinstance(c, Contains) and isinstance(c.lookup.key, Col)]
        if not cands:
            return
        used = []

        def walk(e):
            if isinstance(e, PayloadField):
                used.append(repr(e.lookup)); walk(e.lookup.key)
            elif isinstance(e, Lookup):
                used.append(repr(e)); walk(e.key)
            elif isinstance(e, RecordCons):
                for _, x in e.fields:
                    walk(x)
            elif isinstance(e, (Bin, Cmp)):
                walk(e.left); walk(e.right)
            elif isinstance(e, Call):
                for x in e.args:
                    walk(x)
        walk(op.key); walk(op.val)
        pick = next((c for c in cands if repr(c.lookup) in used), cands[0])
        op.conds = [c for c in op.conds if c is not pick]
        op.probe = pick.lookup

    @staticmethod
    def _only_scalars(e):
        if isinstance(e, (Const, ScalarField)):
            return not isinstance(e, Const) or isinstance(e.value, (int, float))
        if isinstance(e, Bin):
            return _Lowerer._only_scalars(e.left) and _Lowerer._only_scalars(e.right)
        return False

    def _const_str(self, node):
        if isinstance(node, ast.Constant) and isinstance(node.value, str):
            return node.value
        self.fail(node, "expected a string literal")

    def lower(self, fdef):
        self.params = [a.arg for a in fdef.args.args]
        ops, result = [], None
        for st in _desugar(fdef):
            if isinstance(st, ast.Expr) and isinstance(st.value, ast.Constant):
                continue                                    # docstring
            if isinstance(st, ast.Assign) and len(st.targets) == 1 and isinstance(st.targets[0], ast.Name):
                name, val = st.targets[0].id, st.value
                if isinstance(val, ast.Constant):
                    self.consts[name] = val.value
                    continue
                if isinstance(val, ast.Call) and isinstance(val.func, ast.Attribute) and isinstance(val.func.value, ast.Name):
                    ops.append(self.lower_call(name, val))
                    self.dicts.add(name)
                    if isinstance(ops[-1], DistinctOp):
                        self.vectors.add(name)
                    continue
                if isinstance(val, ast.Call) and isinstance(val.func, ast.Name) and val.func.id == "sr_dict" and len(val.args) == 1 \
                        and isinstance(val.args[0], ast.Dict) and len(val.args[0].keys) == 1:
                    k, v = val.args[0].keys[0], val.args[0].values[0]
                    rec = self.expr(k, {})
                    if isinstance(rec, RecordCons) and all(self._only_scalars(e) for _, e in rec.fields) and isinstance(v, ast.Constant) and v.value is True:
                        ops.append(WrapScalarOp(name, rec.fields, st.lineno))
                        self.dicts.add(name)
                        continue
                    self.fail(st, "sr_dict({...}) is only supported as a one-row result {record({name: <scalar>}): True}")
                if isinstance(val, (ast.BinOp, ast.Name, ast.Attribute)):
                    e = self.expr(val, {})
                    if self._only_scalars(e):
                        ops.append(ScalarExprOp(name, e, st.lineno))
                        self.dicts.add(name); self.scalars.add(name)
                        continue
                self.fail(st, "unsupported assignment")
            if isinstance(st, ast.Return):
                if isinstance(st.value, ast.Name) and st.value.id in self.vectors:
                    self.fail(st, "'%s' is a dictionary of sets: it cannot be returned (only dictSize(%s[key]) reads it)" % (st.value.id, st.value.id))
                if isinstance(st.value, ast.Name) and st.value.id in self.dicts:
                    result = st.value.id
                    continue
                self.fail(st, "a query must return one of its results by name")
            self.fail(st, "unsupported statement")
        if result is None:
            raise UnsupportedQuery("%s: no return statement" % self.fn_name)
        return Plan(self.fn_name, self.params, ops, result, dict(self.consts))


def lower_source(source, fn_name=None, first_line=1, outer_consts=None):
    tree = ast.parse(textwrap.dedent(source))
    fdefs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and (fn_name is None or n.name == fn_name)]
    if len(fdefs) != 1:
        raise UnsupportedQuery("expected exactly one function definition")
    return _Lowerer(fdefs[0].name, textwrap.dedent(source).splitlines(), first_line, outer_consts).lower(fdefs[0])


def _outer_constants(func):
    """Numbers and text a query function refers to by a name bound outside it (a parameter of the
    factory that made it, a module-level constant): they are constants of the plan."""
    try:
        cv = inspect.getclosurevars(func)
    except TypeError:
        return {}
    out = {}
    for scope in (cv.globals, cv.nonlocals):
        for name, value in scope.items():
            if isinstance(value, (int, float, str)) and not isinstance(value, bool):
                out[name] = value
    return out


def lower_function(func, in_type=None):
    """Plan for a decorated query function.  ``in_type`` (the decorator's dict) fixes the positional
    order of the table parameters; it must list them in the function's own parameter order."""
    func = getattr(func, "__sdql_func__", func)
    source = inspect.getsource(func)
    first = func.__code__.co_firstlineno
    plan = lower_source(source, func.__name__, first, _outer_constants(func))
    if in_type is not None and len(in_type) != len(plan.params):
        raise UnsupportedQuery("%s: decorator lists %d tables, function takes %d" % (func.__name__, len(in_type), len(plan.params)))
    plan.in_type = in_type
    return plan
