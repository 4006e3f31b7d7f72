"""What the stream tests share: the header's streamed entry points, a recorder for the ctypes handle, a calibrated
stall, and a scanner for the launches in elvis_amd/csrc.  Nothing here touches the GPU at import.

The contract under test: every entry point enqueues on the stream it is given and
on no other, the Python surfaces pass the caller's current stream, and a side stream waits for the current one before it
touches a buffer.
"""
import pathlib
import re
import threading
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "elvis_amd.h"
CSRC = ROOT / "elvis_amd" / "csrc"

STALL_MS = 100.0          # a convention, roughly a thousand small launches; the tests' query() assertions are the condition
STALL_CAP_MS = 500.0      # a convention too: no test may hold the device longer


# ----------------------------------------------------------------------------------------------------------- the header
@dataclass(frozen=True)
class Prototype:
    name: str
    params: Tuple[Tuple[str, str], ...]     # (type, name) in order
    stream: int                             # position of the elvis_stream_t parameter


def _uncomment(src: str) -> str:
    src = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


_PROTO = re.compile(r"\b(?:int|size_t|const\s+char\s*\*)\s*(elvis_\w+)\s*\(([^;{()]*)\)\s*;", re.S)


def prototypes(text: Optional[str] = None) -> List[Tuple[str, Tuple[Tuple[str, str], ...]]]:
    """Every prototype of the header as (name, ((type, name), ...)).  ValueError where something that looks like a
    declaration of an `elvis_` function is not read, or a parameter has no name."""
    src = _uncomment(HEADER.read_text() if text is None else text)
    out = []
    for m in _PROTO.finditer(src):
        args = m.group(2).strip()
        params = []
        if args not in ("", "void"):
            for a in args.split(","):
                pm = re.fullmatch(r"\s*(.*?[\s*&])(\w+)\s*", a, re.S)
                if not pm or not pm.group(1).strip():
                    raise ValueError(f"{m.group(1)}: cannot read the parameter {a.strip()!r}")
                params.append((" ".join(pm.group(1).split()), pm.group(2)))
        out.append((m.group(1), tuple(params)))
    declared = re.findall(r"\b(elvis_\w+)\s*\(", src)
    if sorted(declared) != sorted(name for name, _ in out):
        unread = sorted(set(declared) - {name for name, _ in out}) or sorted(n for n in declared if declared.count(n) > 1)
        raise ValueError(f"include/elvis_amd.h: prototypes that were not read: {unread}")
    return out


def streamed_entry_points(text: Optional[str] = None) -> List[Prototype]:
    """Every prototype with an `elvis_stream_t` parameter, and where it stands.  ValueError for a prototype that cannot
    be read, for one with two streams, and for an `elvis_stream_t` that stands in no prototype (the typedef aside)."""
    src = _uncomment(HEADER.read_text() if text is None else text)
    out = []
    for name, params in prototypes(text):
        at = [i for i, (ty, _) in enumerate(params) if ty == "elvis_stream_t"]
        if len(at) > 1:
            raise ValueError(f"{name}: {len(at)} stream parameters")
        if at:
            out.append(Prototype(name, params, at[0]))
    mentions = len(re.findall(r"\belvis_stream_t\b", src)) - len(re.findall(r"\btypedef\b[^;]*\belvis_stream_t\s*;", src))
    if mentions != len(out):
        raise ValueError(f"include/elvis_amd.h names elvis_stream_t {mentions} times outside its typedef, in {len(out)} prototypes read")
    return out


# ----------------------------------------------------------------------------------------------------------- the recorder
@dataclass(frozen=True)
class Call:
    name: str
    handle: int          # the stream the entry point was given (None counts as 0)
    current: int         # the calling thread's current stream at that moment
    thread: int


def _handle_value(h) -> int:
    if h is None:
        return 0
    v = getattr(h, "value", h)
    return 0 if v is None else int(v)


def _current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


class Recorder:
    """A proxy for the ctypes handle in `elvis_amd._lib._lib`.  A streamed entry point comes back wrapped: the call is
    recorded (name, the handle passed, the calling thread's current stream, the thread) and forwarded.  Every other
    attribute is the handle's own; `restype` and `argtypes` of a wrapped function read and write through."""

    def __init__(self, handle, streamed=None, current: Callable[[], int] = _current_stream):
        protos = streamed_entry_points() if streamed is None else streamed
        object.__setattr__(self, "_handle", handle)
        object.__setattr__(self, "_pos", {p.name: p.stream for p in protos})
        object.__setattr__(self, "_current", current)
        object.__setattr__(self, "_guard", threading.Lock())
        object.__setattr__(self, "calls", [])

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if name not in self._pos:
            return fn
        return _Recorded(self, name, fn)

    def __setattr__(self, name, value):
        setattr(self._handle, name, value)

    def _note(self, name, args):
        pos = self._pos[name]
        if len(args) <= pos:
            raise TypeError(f"{name}: called with {len(args)} arguments, its stream is argument {pos}")
        call = Call(name, _handle_value(args[pos]), int(self._current()), threading.get_ident())
        with self._guard:
            self.calls.append(call)

    def names(self):
        return {c.name for c in self.calls}


class _Recorded:
    def __init__(self, rec, name, fn):
        object.__setattr__(self, "_rec", rec)
        object.__setattr__(self, "_name", name)
        object.__setattr__(self, "_fn", fn)

    def __call__(self, *args):
        self._rec._note(self._name, args)
        return self._fn(*args)

    def __getattr__(self, attr):
        return getattr(self._fn, attr)

    def __setattr__(self, attr, value):
        setattr(self._fn, attr, value)


def install(monkeypatch):
    """Put a Recorder in front of the loaded library for the length of `monkeypatch`'s scope."""
    from elvis_amd import _lib
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    return rec


# ----------------------------------------------------------------------------------------------------------- the stall
_calibration = {}


def calibrate(device):
    """Once a session: how many `torch.cuda._sleep` cycles make a millisecond on `device`, from events.  Where the spin
    kernel does not stall (under 0.2 ms for the probe), the milliseconds one 2048 x 2048 float32 matmul takes instead.
    Returns ("sleep", cycles per ms) or ("matmul", ms per product, the operand)."""
    import torch
    key = str(device)
    if key in _calibration:
        return _calibration[key]
    with torch.cuda.device(device):
        s = torch.cuda.current_stream()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        probe = 20_000_000
        torch.cuda._sleep(1_000_000)                     # the first launch pays for loading the kernel
        s.synchronize()
        start.record(s)
        torch.cuda._sleep(probe)
        end.record(s)
        end.synchronize()
        ms = start.elapsed_time(end)
        if ms >= 0.2:
            _calibration[key] = ("sleep", probe / ms)
        else:
            a = torch.ones((2048, 2048), dtype=torch.float32, device=device)
            (a @ a).sum().item()
            reps = 20
            start.record(s)
            for _ in range(reps):
                a @ a
            end.record(s)
            end.synchronize()
            _calibration[key] = ("matmul", start.elapsed_time(end) / reps, a)
    return _calibration[key]


def stall(stream, ms: float = STALL_MS) -> None:
    """Enqueue about `ms` milliseconds of busy work on `stream` and return at once."""
    import torch
    if not 0 < ms <= STALL_CAP_MS:
        raise ValueError(f"stall: {ms} ms is not within (0, {STALL_CAP_MS}]")
    cal = calibrate(stream.device)
    with torch.cuda.stream(stream):
        if cal[0] == "sleep":
            torch.cuda._sleep(int(cal[1] * ms))
        else:
            _, each, a = cal
            for _ in range(max(1, int(ms / each + 0.5))):
                a @ a


def describe_calibration(device) -> str:
    cal = calibrate(device)
    return f"{cal[1]:.0f} cycles per ms (torch.cuda._sleep)" if cal[0] == "sleep" else f"{cal[1]:.3f} ms per 2048^2 matmul (the spin kernel does not stall)"


# ----------------------------------------------------------------------------------------------------------- the launch scanner
@dataclass(frozen=True)
class Launch:
    path: str
    line: int
    api: str             # hipLaunchKernelGGL, hipMemcpyAsync, hipMemsetAsync, or the offending name
    stream: str          # the stream argument as written
    kind: str            # "cast", "parameter", "local", or "" with `problem` set
    problem: str = ""


OTHER_LAUNCH_APIS = ("<<<", "hipLaunchKernel", "hipModuleLaunchKernel", "hipExtLaunchKernel", "hipExtLaunchKernelGGL",
                     "hipExtModuleLaunchKernel", "hipLaunchCooperativeKernel", "hipLaunchCooperativeKernelMultiDevice",
                     "hipLaunchKernelExC", "hipModuleLaunchCooperativeKernel", "hipGraphLaunch", "hipLaunchHostFunc")
SYNCHRONOUS = ("hipDeviceSynchronize",)         # hipMemcpy(, hipMemset(, hipMemcpyToSymbol and their kin: the hipMem* rule below
STREAM_LAST = ("hipMemcpyAsync", "hipMemsetAsync")


def _blank(src: str) -> str:
    """Comments, string and character literals and line continuations as blanks; offsets and line numbers stay."""
    keep_lines = lambda m: re.sub(r"[^\n]", " ", m.group(0))
    src = re.sub(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'", keep_lines, src, flags=re.S)
    return src.replace("\\\n", " \n")


def _top_level_blocks(text: str, path: str):
    """(head_start, body_start, body_end) of every braced block that stands outside all others, `namespace` and
    `extern "C"` blocks being seen through: the functions (and the odd struct).  ValueError on unbalanced braces."""
    blocks, stack, last = [], [], 0
    for i, ch in enumerate(text):
        outside = all(t for t, _, _ in stack)
        if ch == "{":
            if outside:
                head = text[last:i]
                through = bool(re.search(r"\bnamespace\b[\s\w:]*$|\bextern\s*$", head))
                stack.append((through, last, i + 1))
                if through:
                    last = i + 1
            else:
                stack.append((False, -1, i + 1))
        elif ch == "}":
            if not stack:
                raise ValueError(f"{path}: a closing brace without its opening one at offset {i}")
            through, head_start, body_start = stack.pop()
            if all(t for t, _, _ in stack):
                if not through:
                    blocks.append((head_start, body_start, i))
                last = i + 1
        elif ch == ";" and outside:
            last = i + 1
    if stack:
        raise ValueError(f"{path}: {len(stack)} braces are never closed")
    return blocks


def _call_arguments(text: str, open_paren: int):
    """The arguments of the call whose `(` is at `open_paren`, split at the commas that stand inside no parenthesis,
    bracket, brace or angle bracket (angle brackets are counted only outside parentheses; `->` is an arrow).  Returns
    (arguments, offset after the closing parenthesis), or (None, reason)."""
    depth, angle, args, start, i = 0, 0, [], open_paren + 1, open_paren
    while i < len(text):
        ch = text[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                if angle:
                    return None, "angle brackets do not pair"
                args.append(text[start:i].strip())
                return args, i + 1
        elif depth == 1:
            if ch == "<":
                angle += 1
            elif ch == ">" and text[i - 1] != "-":
                angle -= 1
                if angle < 0:
                    return None, "angle brackets do not pair"
            elif ch == "," and angle == 0:
                args.append(text[start:i].strip())
                start = i + 1
        i += 1
    return None, "the call never closes"


def _classify(expr: str, head: str, body_before: str, depth: int = 0):
    """("cast" | "parameter" | "local", "") for a stream expression that is the caller's, ("", why) otherwise."""
    e = " ".join(expr.split())
    if re.fullmatch(r"\(\s*hipStream_t\s*\)\s*stream", e):
        if re.search(r"\b(?:elvis_stream_t|hipStream_t)\s+stream\s*[,)]", head + ")"):
            return "cast", ""
        return "", "`stream` is no stream parameter of the enclosing function"
    if not re.fullmatch(r"[A-Za-z_]\w*", e):
        return "", f"`{e}` is neither (hipStream_t)stream, a hipStream_t parameter nor a local assigned from one"
    if re.search(rf"\bhipStream_t\s+{e}\s*[,)]", head + ")"):
        return "parameter", ""
    decls = re.findall(rf"\bhipStream_t\s+{e}\s*=\s*([^;]*);", body_before)
    if len(decls) != 1:
        return "", f"`{e}` is declared as a hipStream_t {len(decls)} times in the enclosing function before its use"
    if re.search(rf"(?<![\w.>]){e}\s*=(?!=)", re.sub(rf"\bhipStream_t\s+{e}\s*=", "", body_before)):
        return "", f"`{e}` is assigned again after its declaration"
    if depth > 3:
        return "", f"`{e}`: too long a chain of locals"
    kind, why = _classify(decls[0], head, body_before, depth + 1)
    return ("local", "") if kind else ("", f"`{e}` = `{' '.join(decls[0].split())}`: {why}")


def scan_source(src: str, path: str = "<string>") -> List[Launch]:
    """Every launch, asynchronous copy and fill of one source with its stream classified, and every use of another launch
    API or of a synchronous call as an entry with `problem` set.  An entry that cannot be classified has `problem` set:
    it is a defect, never a pass."""
    text = _blank(src)
    blocks = _top_level_blocks(text, path)
    line = lambda at: text.count("\n", 0, at) + 1

    def enclosing(at):
        for head_start, body_start, body_end in blocks:
            if body_start <= at < body_end:
                return text[head_start:body_start], text[body_start:at]
        return None

    out = []
    for m in re.finditer(r"\b(hipLaunchKernelGGL|hipMem(?:cpy|set)\w*)\s*\(", text):
        api, at = m.group(1), m.start()
        if api != "hipLaunchKernelGGL" and api not in STREAM_LAST:
            out.append(Launch(path, line(at), api, "", "", f"{api}: only {' and '.join(STREAM_LAST)} take the caller's stream"))
            continue
        args, end = _call_arguments(text, m.end() - 1)
        if args is None:
            out.append(Launch(path, line(at), api, "", "", f"cannot read the call: {end}"))
            continue
        if api == "hipLaunchKernelGGL":
            if len(args) < 5:
                out.append(Launch(path, line(at), api, "", "", f"{len(args)} arguments, the stream is the fifth"))
                continue
            expr = args[4]
        else:
            expr = args[-1]
        where = enclosing(at)
        if where is None:
            out.append(Launch(path, line(at), api, expr, "", "stands in no function"))
            continue
        kind, why = _classify(expr, *where)
        out.append(Launch(path, line(at), api, expr, kind, why))
    for api in OTHER_LAUNCH_APIS + SYNCHRONOUS:
        pattern = re.escape(api) if api == "<<<" else rf"\b{api}\b"
        for m in re.finditer(pattern, text):
            out.append(Launch(path, line(m.start()), api, "", "", f"{api} is not allowed in csrc: launches go through hipLaunchKernelGGL on the caller's stream"))
    return out


def csrc_files():
    return sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".inc", ".h"))


def scan_tree() -> List[Launch]:
    out = []
    for p in csrc_files():
        out.extend(scan_source(p.read_text(), f"csrc/{p.name}"))
    return out
