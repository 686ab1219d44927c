"""The workspace ledger read two ways: the user table in the comment at the top of csrc/workspace.hpp, and the ws_reserve call sites
of csrc/.  tests/test_ws_ledger_host.py holds one against the other; tests/test_gpu_recycled_memory.py takes its list of
(slot, entry point) pairs from the table."""
import os
import re

from conftest import REPO

CSRC = os.path.join(REPO, "python-visual-similarity_amd", "csrc")
_FILE = re.compile(r"\b([a-z0-9_]+\.(?:hip|hpp)):")
_FUNCTION = re.compile(r"\b[a-z][a-z0-9]*_[a-z0-9_]+\b")          # every function here has an underscore; the table's prose words have none


def slot_names():
    with open(os.path.join(CSRC, "workspace.hpp")) as f:
        enum = re.search(r"enum WsSlot : int \{(.*?)\};", f.read(), flags=re.S).group(1)
    return [n for n, _ in sorted(re.findall(r"(WS_[A-Z0-9_]+) = (\d+)", enum), key=lambda kv: int(kv[1]))]


def table():
    """-> {slot: {file: [function, ...]}} as the comment table states it.  A row starts with one or more slot names; `file:` opens a
    file's functions; what stands in parentheses is a note."""
    with open(os.path.join(CSRC, "workspace.hpp")) as f:
        text = f.read()
    head = text[text.index("keep the table in step"):text.index("enum WsSlot")]
    lines = [l[2:] for l in head.splitlines()[1:] if l.startswith("//")]
    rows, cur = [], None
    for line in lines:
        m = re.match(r"\s+((?:WS_[A-Z0-9_]+(?:,\s*)?)+)\s+(.*)", line)
        if m:
            cur = [re.findall(r"WS_[A-Z0-9_]+", m.group(1)), m.group(2)]
            rows.append(cur)
        elif cur is not None:
            cur[1] += " " + line.strip()
    out = {}
    for slots, body in rows:
        body = re.sub(r"\([^()]*\)", " ", body)                          # notes
        pieces = _FILE.split(body)                                       # ['', file, functions, file, functions, ...]
        assert not _FUNCTION.search(pieces[0]), f"{slots}: a function before any file name: {pieces[0]!r}"
        for file, funcs in zip(pieces[1::2], pieces[2::2]):
            names = [n for n in _FUNCTION.findall(funcs) if not n.endswith(("_hip", "_hpp"))]
            for slot in slots:
                have = out.setdefault(slot, {}).setdefault(file, [])
                have += [n for n in names if n not in have]
    return out


def table_pairs():
    """-> sorted (slot, function) pairs of the table"""
    return sorted({(slot, fn) for slot, files in table().items() for fns in files.values() for fn in fns})


def reserve_sites():
    """-> {(file, slot): [line numbers]} of every ws_reserve(ctx, WS_X, ...) call under csrc/ (bench/ holds no kernels of the library)"""
    sites = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp")) or name == "workspace.hpp":
            continue
        with open(os.path.join(CSRC, name)) as f:
            for no, line in enumerate(f, 1):
                code = line.split("//")[0]
                for m in re.finditer(r"\bws_reserve\s*\(\s*([A-Za-z_0-9>-]+)\s*,\s*([A-Za-z_0-9:]+)", code):
                    if re.match(r"\s*(int|inline)\b", code):             # the definition in api.hip
                        continue
                    sites.setdefault((name, m.group(2)), []).append(no)
    return sites
