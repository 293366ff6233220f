"""The upload discipline of stark_mlwe_amd/csrc, checked on the sources ("Uploads"): host memory reaches the device in three functions and
nowhere else — ctx_upload_staged (the context owns a copy), CallerUploads::copy (the fence guard of the caller's arrays) and DevMem::fill_sync (copy
and synchronise).  A plain text search for the project's own names; no GPU."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stark_mlwe_amd", "csrc")
KIND = "hipMemcpyHostToDevice"
ALLOWED = {"ctx_upload_staged", "copy", "fill_sync"}
# a definition's head: `name(args) {` or `name(args) const {`, the name possibly qualified (DevMem::fill_sync)
HEAD = re.compile(r"(?:\w+::)?(\w+)\s*\([^(){};]*\)\s*(?:const\s*)?\{")
KEYWORDS = {"if", "for", "while", "switch", "return", "sizeof", "catch"}


def sources():
    files = sorted(f for pat in ("*.hip", "*.hpp", "*.cpp", "*.inc") for f in glob.glob(os.path.join(CSRC, pat)))
    assert files, "no sources under " + CSRC
    return [(os.path.basename(f), open(f).read().split("\n")) for f in files]


def enclosing_function(lines, i, col):
    """the name of the innermost function definition whose head stands before column `col` of line i, or at the start of an unindented line above"""
    heads = [m.group(1) for m in HEAD.finditer(lines[i][:col]) if m.group(1) not in KEYWORDS]
    if heads:
        return heads[-1]
    for j in range(i - 1, -1, -1):
        if lines[j][:1] not in ("", " ", "\t", "/", "#", "}"):
            heads = [m.group(1) for m in HEAD.finditer(lines[j]) if m.group(1) not in KEYWORDS]
            return heads[0] if heads else None
    return None


def test_the_parser_names_what_it_should():
    lines = ["int32_t ctx_upload_staged(stark_ctx* ctx, void* dst, const void* src, size_t bytes) {", "    if (!bytes) return STARK_OK;", "    STARK_HIP(ctx, copy_it(dst, X, s));", "}",
             "struct G {", "    hipError_t copy(void* dst, size_t bytes) { if (!bytes) return hipSuccess; return go(dst, X); }", "};",
             "inline int32_t DevMem::fill_sync(stark_ctx* ctx, void* dst) {", "    go(X); return 0;", "}",
             "int32_t stark_thing(stark_ctx_t* ctx, void* d) {", "    if (!ctx) return -1;", "    go(X); }"]
    where = [enclosing_function(lines, i, l.index("X")) for i, l in enumerate(lines) if "X" in l]
    assert where == ["ctx_upload_staged", "copy", "fill_sync", "stark_thing"]


def test_host_to_device_copies_only_in_the_three_functions():
    found = []
    for name, lines in sources():
        for i, l in enumerate(lines):
            for m in re.finditer(KIND, l):
                found.append((name, i + 1, enclosing_function(lines, i, m.start())))
    assert found, "no host-to-device copy found at all: the search itself is broken"
    outside = [f for f in found if f[2] not in ALLOWED]
    assert not outside, "host-to-device copies outside ctx_upload_staged / CallerUploads::copy / DevMem::fill_sync: %s" % outside
    assert {f[2] for f in found} == ALLOWED, "expected one site in each of the three functions, found %s" % found
    assert {(f[0], f[2]) for f in found} == {("capi_core.hip", "ctx_upload_staged"), ("ctx.hpp", "copy"), ("ctx.hpp", "fill_sync")}, found


def struct_body(text, name):
    m = re.search(r"\bstruct\s+%s\b[^;{]*\{" % name, text)
    assert m, "struct %s not found" % name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0); i += 1
    return text[m.end():i - 1]


def test_devbuf_has_no_upload_member_and_the_guard_owns_the_copy():
    ctx_hpp = open(os.path.join(CSRC, "ctx.hpp")).read()
    assert not re.search(r"\bupload\s*\(", struct_body(ctx_hpp, "DevBuf")), "DevBuf has an upload member again: use ctx_upload_staged or a CallerUploads guard"
    assert KIND in struct_body(ctx_hpp, "CallerUploads")
    assert "ctx_upload_staged" in struct_body(ctx_hpp, "DevArena") and KIND not in struct_body(ctx_hpp, "DevArena")


def test_sumcheck_executor_has_no_staging_list_of_its_own():
    text = open(os.path.join(CSRC, "capi_sumcheck.hip")).read()
    assert not re.search(r"\bstaged\b", text), "capi_sumcheck.hip declares or uses a `staged` member: the executors' uploads go through DevArena"
    assert re.search(r"struct\s+ScDevExec\s*:\s*DevArena\b", text)
