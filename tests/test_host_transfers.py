"""Every device transfer of the host layer goes through the transfer helpers of msdr_api.hip ("Transfers"): they enqueue on the
context's stream, so a copy or a clear is ordered behind whatever the stream already holds.  A bare hipMemcpy / hipMemset on the null stream
is not (the context's stream is non-blocking): that race once made the first input-row map of a process read as zeros.

The comment-stripped text of every .hip / .hiph / .h / .cpp under minimal-sdr_amd/csrc is searched for calls of hipMemcpy*, hipMemset* (the
Async, 2D, ... variants included).  A call is in order inside one of the named helpers, or where ALLOWED lists it with its reason.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
API = "msdr_api.hip"
HELPERS = ("copy_in_nowait", "copy_in", "copy_in_2d", "copy_out", "copy_dev", "fill_dev")
CALL = re.compile(r"\bhip(?:Memcpy|Memset)\w*\s*\(")
# (file, the call's text from its name on, how often, why it may stand outside the helpers)
ALLOWED = (
    (API, "hipMemcpyAsync((char *)d_recv + (size_t)root * local_bytes, d_local, local_bytes, hipMemcpyDeviceToDevice, C->stream)", 1,
     "msdr_gather_audio_begin: the root's own shard, on the communicator's stream behind its ready event"),
    (API, "hipMemsetAsync(stamp_buf, 0, stamp_n * 8, c->ctx->stream)", 1, "MSDR_STAMPS diagnostic build: clears the cycle stamps on the chain's stream"),
    (API, "hipMemcpy(h.data(), p.dbg_buf, h.size() * 8, hipMemcpyDeviceToHost)", 1, "MSDR_STAMPS diagnostic build: reads the stamps behind a stream synchronisation"),
    ("msdr_chain_block.hip", "hipMemsetAsync(stamp_buf, 0, stamp_n * 8, stream)", 1, "MSDR_MB_STAMPS diagnostic build: the launcher has a stream, no context"),
    ("msdr_chain_block.hip", "hipMemcpy(h.data(), stamp_buf, h.size() * 8, hipMemcpyDeviceToHost)", 1, "MSDR_MB_STAMPS diagnostic build: behind a stream synchronisation"),
)


def strip_comments(text):
    """C++ text without its comments; string and character literals stay (a call's name inside a literal would still be flagged: none exists)"""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if text.startswith("//", i):
            i = text.find("\n", i)
            i = n if i < 0 else i
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            out.append("\n" * text.count("\n", i, n if j < 0 else j))
            i = n if j < 0 else j + 2
        elif ch in "\"'":
            j = i + 1
            while j < n and text[j] != ch:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        else:
            out.append(ch)
            i += 1
    return "".join(out)


def call_text(text, at):
    """the call that starts at `at`, up to its closing parenthesis, white space squeezed"""
    depth, j = 0, text.index("(", at)
    while True:
        depth += {"(": 1, ")": -1}.get(text[j], 0)
        j += 1
        if depth == 0:
            return " ".join(text[at:j].split())


def helper_spans(text):
    """[start, end) of each named helper's definition in msdr_api.hip"""
    spans = []
    for name in HELPERS:
        hits = list(re.finditer(r"\bstatic\s+hipError_t\s+%s\s*\([^)]*\)\s*\{" % name, text))
        assert len(hits) == 1, (name, len(hits))
        depth, j = 1, hits[0].end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[j], 0)
            j += 1
        spans.append((hits[0].start(), j))
    return spans


def bare_calls(fname, text):
    """-> [(line, call text)] of the transfer calls outside the helpers"""
    text = strip_comments(text)
    spans = helper_spans(text) if fname == API else []
    return [(text.count("\n", 0, m.start()) + 1, call_text(text, m.start())) for m in CALL.finditer(text)
            if not any(a <= m.start() < b for a, b in spans)]


def sources():
    for base, _, files in sorted(os.walk(CSRC)):
        for f in sorted(files):
            if f.endswith((".hip", ".hiph", ".h", ".cpp")):
                with open(os.path.join(base, f)) as fh:
                    yield os.path.relpath(os.path.join(base, f), CSRC), fh.read()


def test_every_transfer_goes_through_the_helpers():
    found = [(f, line, call) for f, text in sources() for line, call in bare_calls(f, text)]
    allowed = {(f, call): count for f, call, count, _ in ALLOWED}
    stray = [(f, line, call) for f, line, call in found if (f, call) not in allowed]
    assert not stray, "bare transfer calls (use copy_in / copy_out / copy_dev / copy_in_2d / copy_in_nowait / fill_dev):\n" + "\n".join("%s:%d: %s" % s for s in stray)
    for (f, call), count in allowed.items():          # (an entry nothing matches any more has to leave the list)
        assert sum(1 for g, _, c in found if (g, c) == (f, call)) == count, (f, call)
    assert all(reason for _, _, _, reason in ALLOWED)


def test_each_helper_makes_exactly_one_transfer_call_on_the_contexts_stream():
    text = strip_comments(dict(sources())[API])
    for (a, b), name in zip(helper_spans(text), HELPERS):
        body = text[a:b]
        calls = CALL.findall(body)
        assert len(calls) == (0 if name == "copy_in" else 1), (name, calls)          # (copy_in is copy_in_nowait and the wait)
        assert "ctx->stream" in body or name == "copy_in", name
        assert ("hipStreamSynchronize" in body or "waited(" in body) == (name in ("copy_in", "copy_in_2d", "copy_out")), name


def test_the_scan_sees_a_bare_call_a_commented_one_it_does_not():
    api = dict(sources())[API]
    planted = api + "\nstatic int planted(void *d, const void *s) { /* hipMemset(d, 0, 4); */ return (int)hipMemcpy (d, s, 4,\n hipMemcpyHostToDevice); }  // hipMemcpyAsync(\n"
    extra = [c for c in bare_calls(API, planted) if c not in bare_calls(API, api)]
    assert extra == [(api.count("\n") + 2, "hipMemcpy (d, s, 4, hipMemcpyHostToDevice)")], extra
    assert bare_calls("other.h", "inline void f(void *d) { (void)hipMemsetD32Async((hipDeviceptr_t)d, 0, 1, nullptr); }") == \
        [(1, "hipMemsetD32Async((hipDeviceptr_t)d, 0, 1, nullptr)")]
