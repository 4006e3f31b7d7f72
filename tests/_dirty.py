"""Poison fresh allocations, and list where the package makes them.

`poison` replaces `torch.empty`, `torch.empty_like` and `Tensor.new_empty` for one
test: each still allocates, then every byte of the result is set to one value, so a
kernel that reads an element nobody wrote reads that value and not the zero (or the
previous test's right answer) the allocator happened to hand back.  Two bytes are
used; what they read as is `READS_AS` below.  A sum that swallows one of them cannot
swallow the other.

`sites` is the other half: an `ast` scan of the package for every spelling that can
reach one of the three allocators, keyed without line numbers.
"""
import ast
import pathlib
import struct
import sys

import torch

PKG = pathlib.Path(__file__).resolve().parent.parent / "elvis_amd"
POISONS = (0xFF, 0x7F)
CALLEES = ("torch.empty", "torch.empty_like", "new_empty")



def _reads_as(byte):
    f = lambda fmt, n: struct.unpack(fmt, bytes([byte]) * n)[0]
    clean = lambda v: None if v != v else v            # NaN spelt None
    return {torch.float16: clean(f("<e", 2)), torch.float32: clean(f("<f", 4)), torch.float64: clean(f("<d", 8)),
            torch.int8: f("<b", 1), torch.int32: f("<i", 4), torch.int64: f("<q", 8), torch.uint8: byte}


# what a tensor filled with the byte reads as, from the number formats alone; the ledger's self-test walks this
READS_AS = {byte: _reads_as(byte) for byte in POISONS}


def _fill(t, byte):
    if t.numel():
        t.reshape(-1).view(torch.uint8).fill_(byte)
        if t.is_cuda:             # the fill is on the current stream: done before a side stream can be handed the tensor
            torch.cuda.current_stream(t.device).synchronize()
    return t


_SCOPES = {}   # file -> {(co_name, co_firstlineno): qualified name}, for interpreters without co_qualname


def _site(frame):
    code = frame.f_code
    module = frame.f_globals.get("__name__", "?")
    if hasattr(code, "co_qualname"):
        return module, code.co_qualname
    if code.co_filename not in _SCOPES:
        scan = _Scan(module)
        try:
            scan.visit(ast.parse(pathlib.Path(code.co_filename).read_text()))
        except (OSError, SyntaxError):
            pass
        _SCOPES[code.co_filename] = scan.scopes
    return module, _SCOPES[code.co_filename].get((code.co_name, code.co_firstlineno), code.co_name)


def poison(monkeypatch, byte):
    """Patch the three allocators; returns the set of (module, qualified function, callee) that ran."""
    seen = set()
    real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def empty(*a, **k):
        seen.add(_site(sys._getframe(1)) + ("torch.empty",))
        return _fill(real_empty(*a, **k), byte)

    def empty_like(*a, **k):
        seen.add(_site(sys._getframe(1)) + ("torch.empty_like",))
        return _fill(real_like(*a, **k), byte)

    def new_empty(self, *a, **k):
        seen.add(_site(sys._getframe(1)) + ("new_empty",))
        return _fill(real_new(self, *a, **k), byte)

    monkeypatch.setattr(torch, "empty", empty)
    monkeypatch.setattr(torch, "empty_like", empty_like)
    monkeypatch.setattr(torch.Tensor, "new_empty", new_empty)
    return seen


class _Scan(ast.NodeVisitor):
    def __init__(self, module):
        self.module, self.stack, self.found, self.scopes, self.counts = module, [], set(), {}, {}

    def _enter(self, name, line):
        self.stack += [name, "<locals>"]
        self.scopes[(name, line)] = self._where()

    def _scope(self, node):
        self.stack.append(node.name)
        self.generic_visit(node)
        self.stack.pop()

    def visit_ClassDef(self, node):
        self._scope(node)

    def visit_FunctionDef(self, node):
        for d in node.decorator_list:      # decorators run in the enclosing scope
            self.visit(d)
        self._enter(node.name, min([node.lineno] + [d.lineno for d in node.decorator_list]))
        for part in [node.args, node.returns] + node.body:
            if part is not None:
                self.visit(part)
        del self.stack[-2:]

    visit_AsyncFunctionDef = visit_FunctionDef

    def visit_Lambda(self, node):
        self._enter("<lambda>", node.lineno)
        self.generic_visit(node)
        del self.stack[-2:]

    def _comp(self, node):
        # before 3.12 a comprehension is a frame of its own; the poisoner sees that frame's name
        if sys.version_info < (3, 12):
            kind = {"ListComp": "<listcomp>", "SetComp": "<setcomp>", "DictComp": "<dictcomp>", "GeneratorExp": "<genexpr>"}
            self._enter(kind[type(node).__name__], node.lineno)
            self.generic_visit(node)
            del self.stack[-2:]
        elif isinstance(node, ast.GeneratorExp):
            self._enter("<genexpr>", node.lineno)
            self.generic_visit(node)
            del self.stack[-2:]
        else:
            self.generic_visit(node)

    visit_ListComp = visit_SetComp = visit_DictComp = visit_GeneratorExp = _comp

    def _where(self):
        s = self.stack[:-1] if self.stack and self.stack[-1] == "<locals>" else self.stack
        return ".".join(s) if s else "<module>"

    def visit_Attribute(self, node):
        # a call and a bare reference both pass here: `torch.empty(...)`, `f = torch.empty`, `x.new_empty(...)`
        site = None
        if node.attr in ("empty", "empty_like") and isinstance(node.value, ast.Name) and node.value.id == "torch":
            site = (self.module, self._where(), "torch." + node.attr)
        elif node.attr == "new_empty":
            site = (self.module, self._where(), "new_empty")
        if site is not None:
            self.found.add(site)
            self.counts[site] = self.counts.get(site, 0) + 1
        self.generic_visit(node)


def site_counts():
    """{(module, qualified function, callee): how many times the function spells it} over elvis_amd/*.py."""
    out = {}
    for path in sorted(PKG.glob("*.py")):
        scan = _Scan("elvis_amd." + path.stem)
        scan.visit(ast.parse(path.read_text(), str(path)))
        out.update(scan.counts)
    return out


def sites():
    """Every (module, qualified function, callee) in elvis_amd/*.py that can reach an allocator."""
    return set(site_counts())
