"""CPU suite: the table of the engine's device buffers (tuatara_amd/csrc/engine.h: kDevBufTable, read through ttr_dbg_scratch_table) names exactly the DevBuf
members the header declares, every kept row says why it is kept, and no buffer the sources read as integers is listed with a float kind (the poison hook of
tests/test_gpu_history.py writes NaN and 1e4 into float rows; an index must only ever see zeros).  No GPU here."""
import glob
import os
import re

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "tuatara_amd", "csrc")
# the structs of engine.h that own device buffers, and the prefix their members carry in the table
OWNER_PREFIX = {"Engine": "", "CclBatch": "ccl.", "Linear": "linear.", "HeadTail": "head_tail.", "Comm": "comm."}


@pytest.fixture(scope="module")
def table():
    from tuatara_amd import build
    build.build_all()
    from tuatara_amd import engine
    return engine.scratch_table()


def _strip_comments(src: str) -> str:
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def declared_devbufs(src: str):
    """Every DevBuf member a header declares, as the table names it: plain members, arrays (`pq_ws[kWsCount]`), comma lists (`DevBuf w, b;`), containers
    (`std::map<std::string, DevBuf> pqf;`, `std::vector<std::unique_ptr<DevBuf>> craft_ws_set[2];`), each under the innermost struct that encloses it."""
    src = _strip_comments(src)
    decl = re.compile(r"[;{}]\s*(?:(?:static|mutable)\s+)?((?:std::[\w:<>,\s]*[<,]\s*)?DevBuf(?:\s*>)*)\s+([A-Za-z_][^;(){}]*)(?=;)")
    opens = {m.end() - 1: m.group(1) for m in re.finditer(r"\bstruct\s+(\w+)[^;{}()]*\{", src)}   # position of a struct's '{' -> its name
    hits = {m.start(2): m.group(2) for m in decl.finditer(src)}
    names, stack = [], []
    for i, ch in enumerate(src):
        if ch == "{":
            stack.append(opens.get(i))
        elif ch == "}":
            stack.pop()
        if i in hits:
            owner = next((s for s in reversed(stack) if s), None)
            assert owner in OWNER_PREFIX, f"DevBuf members inside struct {owner}: give the struct a prefix here and its members rows in kDevBufTable"
            for part in hits[i].split(","):
                name = re.sub(r"\[[^\]]*\]", "", part.split("=")[0]).strip()
                assert re.fullmatch(r"[A-Za-z_]\w*", name), (hits[i], name)
                names.append(OWNER_PREFIX[owner] + name)
    return names


def test_the_parser_reads_arrays_lists_containers_and_nested_structs():
    src = """
    struct DevBuf { void* p; DevBuf() = default; DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete; };
    struct Linear { DevBuf w, b;   // a list
      DevBuf ws; };
    struct Engine {
      struct HeadTail { DevBuf w6, w8; float s6 = 0; } head_tail;
      std::map<std::string, DevBuf> pqf;   /* a container */
      std::vector<std::unique_ptr<DevBuf>> craft_ws_set[2];
      DevBuf pq_ws[kWsCount];
      DevBuf a, b[2], c;
      static RecOut rec_block(DevBuf& d, int rows) { return RecOut{}; }
      DevBuf& ws(size_t idx);
      void upload_f32(DevBuf& d, const float* p);
    };"""
    assert declared_devbufs(src) == ["linear.w", "linear.b", "linear.ws", "head_tail.w6", "head_tail.w8", "pqf", "craft_ws_set", "pq_ws", "a", "b", "c"]
    with pytest.raises(AssertionError, match="struct Other"):
        declared_devbufs("struct Other { DevBuf x; };")


def test_the_table_names_exactly_the_declared_device_buffers(table):
    declared = declared_devbufs(open(os.path.join(CSRC, "engine.h")).read())
    assert len(declared) == len(set(declared)), sorted(n for n in declared if declared.count(n) > 1)
    assert len(declared) >= 80     # (the parser found the header's members at all)
    listed = [r[0] for r in table]
    assert len(listed) == len(set(listed)), sorted(n for n in listed if listed.count(n) > 1)
    assert sorted(set(declared) - set(listed)) == [], "device buffers without a row in kDevBufTable"
    assert sorted(set(listed) - set(declared)) == [], "rows of kDevBufTable that engine.h no longer declares"
    # no other file of the engine owns a DevBuf member: locals of the developer hooks aside, the header is the whole list
    for path in glob.glob(os.path.join(CSRC, "*.h")):
        if os.path.basename(path) != "engine.h":
            assert not re.search(r"\bDevBuf\b", _strip_comments(open(path).read())), path


def test_every_row_has_a_class_and_a_kind_and_every_kept_row_a_contract(table):
    for name, cls, kind, note in table:
        assert cls in ("scratch", "kept"), (name, cls)
        assert kind in ("f32", "f16", "u8", "i32", "addr"), (name, kind)
        if cls == "kept":
            assert len(note.split()) >= 5 and note[0].isalpha(), f"{name}: a kept row states the contract that makes it so"
    # the buffers whose contents are contracts, by name: none of them may be poisoned
    cls_of = {r[0]: r[1] for r in table}
    for name in ("linear.w", "linear.b", "linear.ws", "linear.wst", "linear.wsp", "pqf", "qself", "lex_records", "pattern_dev", "dsk_cs", "range_word", "ar_done",
                 "head_tail.w6", "head_tail.w8", "head_tail.b6", "head_tail.b8"):
        assert cls_of[name] == "kept", name
    # the two write-once float buffers live inside scratch rows: their rows say so
    note_of = {r[0]: r[3] for r in table}
    assert "zero_new" in note_of["craft_ws_set"] and "kept" in note_of["craft_ws_set"]
    assert "kWsKvcache" in note_of["pq_ws"] and "kept" in note_of["pq_ws"]


def test_no_buffer_read_as_integers_is_listed_with_a_float_kind(table):
    """A member the sources view as integers (`x.as<int>()`, `.as<unsigned>()`, `.as<int64_t>()` ...) holds indices, counters or records: its row must be i32
    (or addr), so that the poison only ever writes zeros into it."""
    ints = set()
    view = re.compile(r"\b([A-Za-z_]\w*)(?:\[[^\]]*\])?\s*\.\s*as<\s*(?:const\s+)?(?:unsigned\s+long\s+long|unsigned|int|long\s+long|u?int(?:32|64)_t|size_t)\s*>")
    for path in glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.h")):
        ints.update(view.findall(_strip_comments(open(path).read())))
    assert {"parent", "counters", "tokens", "lex_side"} <= ints      # (the scan sees the engine's integer views)
    rows = {r[0].split(".")[-1]: r for r in table}
    bad = [(r[0], r[2]) for short, r in rows.items() if short in ints and r[2] in ("f32", "f16")]
    assert bad == []
    # address rows: the page tables hold device pointers and are never filled
    for name in ("page_table", "tile_table", "dsk_table"):
        assert {r[0]: r[2] for r in table}[name] == "addr"
