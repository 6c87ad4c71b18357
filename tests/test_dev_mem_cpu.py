"""The owner of a context's allocations (freud_amd/csrc/dev_mem.h) compiled for the HOST (g++ -Wall -Werror) into a stand-alone
program over a malloc backend.  The backend numbers its blocks, keeps the set of live ones with the kind that allocated each, and
ABORTS on a double free, an unknown pointer or a free by another kind's function; it can be told to fail its k-th allocation.  Every
scenario prints the backend's events and the owner's state; the tests below assert on that log.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include "dev_mem.h"

struct Block { int id, kind; size_t bytes; };
static std::map<void*, Block> g_live;
static int g_next_id = 1, g_allocs = 0, g_fail_at = 0;
static void** g_watch = nullptr;            // a field whose value every allocation reports (null before the new block arrives?)

template <int KIND>
static const char* be_alloc(void** p, size_t bytes) {
  ++g_allocs;
  if (g_allocs == g_fail_at) {
    printf("ev fail kind=%d bytes=%zu watch_null=%d\n", KIND, bytes, g_watch ? *g_watch == nullptr : -1);
    return "out of memory";
  }
  *p = malloc(bytes ? bytes : 1);
  g_live[*p] = Block{g_next_id, KIND, bytes};
  printf("ev alloc kind=%d bytes=%zu id=%d watch_null=%d\n", KIND, bytes, g_next_id, g_watch ? *g_watch == nullptr : -1);
  ++g_next_id;
  return nullptr;
}
template <int KIND>
static void be_free(void* p) {
  auto it = g_live.find(p);
  if (it == g_live.end()) { printf("ABORT free of an unknown or already freed pointer (kind %d)\n", KIND); fflush(stdout); abort(); }
  if (it->second.kind != KIND) { printf("ABORT block of kind %d freed by kind %d\n", it->second.kind, KIND); fflush(stdout); abort(); }
  printf("ev free kind=%d id=%d\n", KIND, it->second.id);
  g_live.erase(it);
  free(p);
}

static void kinds(DevMem& m) {
  m.kinds[DM_DEVICE] = {be_alloc<DM_DEVICE>, be_free<DM_DEVICE>};
  m.kinds[DM_PEER] = {be_alloc<DM_PEER>, be_free<DM_PEER>};
  m.kinds[DM_UNCACHED] = {be_alloc<DM_UNCACHED>, be_free<DM_UNCACHED>};
  m.kinds[DM_PINNED] = {be_alloc<DM_PINNED>, be_free<DM_PINNED>};
  m.kinds[DM_MAPPED] = {be_alloc<DM_MAPPED>, be_free<DM_MAPPED>};
}

static int id_of(void* p) { auto it = g_live.find(p); return p == nullptr ? 0 : it == g_live.end() ? -1 : it->second.id; }
static void state(const char* tag, const DevMem& m) {
  printf("state %s live=%zu recs=%zu", tag, g_live.size(), m.recs.size());
  for (const auto& r : m.recs) printf(" [id=%d bytes=%zu kind=%d]", id_of(*r.field), r.bytes, r.kind);
  printf("\n");
}

struct Ctx { float* a = nullptr; char* b = nullptr; int* c = nullptr; double* d = nullptr; unsigned* e = nullptr; };

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  DevMem m;
  kinds(m);
  Ctx x;
  if (!strcmp(mode, "alloc")) {
    printf("ok %d\n", (int)m.alloc(x.a, 100, DM_DEVICE, "x.a"));
    printf("ok %d\n", (int)m.alloc(x.b, 64, DM_PINNED, "x.b"));
    printf("fields a=%d b=%d\n", id_of(x.a), id_of(x.b));
    printf("rec0_is_a %d rec1_is_b %d\n", m.recs[0].field == (void**)&x.a, m.recs[1].field == (void**)&x.b);
    state("end", m);
    memset(x.a, 1, 100); memset(x.b, 2, 64);            // (the blocks are really there)
    m.free_all();
  } else if (!strcmp(mode, "grow")) {
    g_watch = (void**)&x.a;
    printf("ok %d\n", (int)m.grow(x.a, 100, DM_DEVICE, "x.a"));      // first use: allocates and records
    state("first", m);
    printf("mark same\n");
    printf("ok %d\n", (int)m.grow(x.a, 100, DM_DEVICE, "x.a"));
    printf("mark smaller\n");
    printf("ok %d\n", (int)m.grow(x.a, 10, DM_DEVICE, "x.a"));
    state("kept", m);
    printf("mark larger\n");
    printf("ok %d\n", (int)m.grow(x.a, 101, DM_DEVICE, "x.a"));
    state("grown", m);
    m.free_all();
  } else if (!strcmp(mode, "fail")) {
    g_watch = (void**)&x.a;
    m.alloc(x.b, 32, DM_DEVICE, "x.b");
    m.grow(x.a, 100, DM_DEVICE, "x.a");
    g_fail_at = g_allocs + 1;                            // the next allocation fails: the one inside the grow below
    printf("mark failing\n");
    printf("ok %d\n", (int)m.grow(x.a, 200, DM_DEVICE, "x.a"));
    printf("err %s\n", m.err);
    printf("field_null %d\n", x.a == nullptr);
    state("failed", m);
    printf("mark again\n");
    printf("ok %d\n", (int)m.grow(x.a, 50, DM_DEVICE, "x.a"));       // a size the OLD block would have served: it is gone, so this allocates
    state("again", m);
    printf("ok %d\n", (int)m.alloc(x.c, 8, DM_PEER, "x.c"));         // the owner takes new fields as before
    g_fail_at = g_allocs + 1;
    printf("mark failing_alloc\n");
    printf("ok %d\n", (int)m.alloc(x.d, 16, DM_DEVICE, "x.d"));      // a failing first allocation: null field, size 0
    printf("field_null %d\n", x.d == nullptr);
    printf("ok %d\n", (int)m.grow(x.d, 16, DM_DEVICE, "x.d"));       // ... and a later grow of it succeeds
    state("end", m);
    m.free_all();
    state("freed", m);
  } else if (!strcmp(mode, "free_all")) {
    m.alloc(x.a, 100, DM_DEVICE, "x.a");
    m.alloc(x.b, 10, DM_PEER, "x.b");
    m.alloc(x.c, 20, DM_UNCACHED, "x.c");
    m.alloc(x.d, 30, DM_PINNED, "x.d");
    m.alloc(x.e, 40, DM_MAPPED, "x.e");
    state("full", m);
    printf("mark free_all\n");
    m.free_all();
    printf("fields_null %d\n", !x.a && !x.b && !x.c && !x.d && !x.e);
    state("freed", m);
    printf("mark second\n");
    m.free_all();
    state("second", m);
    printf("ok %d\n", (int)m.grow(x.a, 5, DM_DEVICE, "x.a"));        // an emptied owner serves again
    m.free_all();
    state("end", m);
  } else if (!strcmp(mode, "backend_double_free")) {                  // the backend's own guard: must abort
    void* p = nullptr;
    be_alloc<0>(&p, 8);
    be_free<0>(p);
    be_free<0>(p);
  } else if (!strcmp(mode, "backend_wrong_kind")) {
    void* p = nullptr;
    be_alloc<DM_PINNED>(&p, 8);
    be_free<DM_DEVICE>(p);
  } else {
    return 2;
  }
  return 0;
}
"""


def _build(d, extra=()):
    src = d / "dev_mem.cpp"
    src.write_text(_SRC)
    exe = d / ("dev_mem" + ("_san" if extra else ""))
    done = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)],
                          capture_output=True, text=True)
    return (str(exe) if done.returncode == 0 else None), done.stderr


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("dev_mem")
    exe, err = _build(d)
    assert exe, err
    return {"plain": exe, "dir": d}


def _sanitized(exes):
    """The same program under the host's address and undefined-behaviour sanitizers, or None where this g++ does not link them."""
    if "san" not in exes:
        exes["san"] = _build(exes["dir"], ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))[0]
    return exes["san"]


def _run(exe, mode):
    done = subprocess.run([exe, mode], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    return done.stdout.split("\n")[:-1]


def _runs(exes, mode):
    """The scenario's log from the plain program -- and, where the sanitizers link, from the sanitized one, which must agree."""
    log = _run(exes["plain"], mode)
    san = _sanitized(exes)
    if san:
        assert _run(san, mode) == log
    return log


def _between(log, a, b=None):
    i = log.index(f"mark {a}")
    j = log.index(f"mark {b}") if b else len(log)
    return log[i + 1:j]


def _events(lines):
    return [ln for ln in lines if ln.startswith("ev ")]


def test_alloc_stores_and_records(exes):
    log = _runs(exes, "alloc")
    assert log[:6] == ["ev alloc kind=0 bytes=100 id=1 watch_null=-1", "ok 1", "ev alloc kind=3 bytes=64 id=2 watch_null=-1", "ok 1",
                       "fields a=1 b=2", "rec0_is_a 1 rec1_is_b 1"]
    assert log[6] == "state end live=2 recs=2 [id=1 bytes=100 kind=0] [id=2 bytes=64 kind=3]"


def test_grow_with_a_sufficient_size_touches_nothing(exes):
    log = _runs(exes, "grow")
    assert "state first live=1 recs=1 [id=1 bytes=100 kind=0]" in log
    assert _between(log, "same", "smaller") == ["ok 1"]                     # no event at all: neither a free nor an allocation
    assert _between(log, "smaller", "larger") == ["ok 1", "state kept live=1 recs=1 [id=1 bytes=100 kind=0]"]


def test_grow_frees_exactly_the_old_block_and_nulls_the_field_before_allocating(exes):
    log = _runs(exes, "grow")
    larger = _between(log, "larger")
    assert larger[:3] == ["ev free kind=0 id=1", "ev alloc kind=0 bytes=101 id=2 watch_null=1", "ok 1"]
    assert larger[3] == "state grown live=1 recs=1 [id=2 bytes=101 kind=0]"


def test_failed_allocation_leaves_null_and_zero_and_the_owner_usable(exes):
    log = _runs(exes, "fail")
    failing = _between(log, "failing", "again")
    assert failing[:2] == ["ev free kind=0 id=2", "ev fail kind=0 bytes=200 watch_null=1"]
    assert failing[2:5] == ["ok 0", "err hipMalloc(200 bytes) for x.a failed: out of memory", "field_null 1"]
    assert failing[5] == "state failed live=1 recs=2 [id=1 bytes=32 kind=0] [id=0 bytes=0 kind=0]"
    again = _between(log, "again", "failing_alloc")
    assert again[:3] == ["ev alloc kind=0 bytes=50 id=3 watch_null=1", "ok 1",
                         "state again live=2 recs=2 [id=1 bytes=32 kind=0] [id=3 bytes=50 kind=0]"]
    assert again[3:] == ["ev alloc kind=1 bytes=8 id=4 watch_null=0", "ok 1"]
    tail = _between(log, "failing_alloc")
    assert tail[:3] == ["ev fail kind=0 bytes=16 watch_null=0", "ok 0", "field_null 1"]
    assert tail[3:5] == ["ev alloc kind=0 bytes=16 id=5 watch_null=0", "ok 1"]
    assert tail[5] == "state end live=4 recs=4 [id=1 bytes=32 kind=0] [id=3 bytes=50 kind=0] [id=4 bytes=8 kind=1] [id=5 bytes=16 kind=0]"
    assert tail[-1] == "state freed live=0 recs=0"                          # (the failed record of x.d was not freed twice: no abort)


def test_free_all_empties_and_a_second_one_is_a_no_op(exes):
    log = _runs(exes, "free_all")
    assert "state full live=5 recs=5 [id=1 bytes=100 kind=0] [id=2 bytes=10 kind=1] [id=3 bytes=20 kind=2] [id=4 bytes=30 kind=3] [id=5 bytes=40 kind=4]" in log
    first = _between(log, "free_all", "second")
    assert sorted(_events(first)) == [f"ev free kind={k} id={k + 1}" for k in range(5)]
    assert first[-2:] == ["fields_null 1", "state freed live=0 recs=0"]
    second = _between(log, "second")
    assert second[0] == "state second live=0 recs=0"                        # no event before it
    assert second[1:] == ["ev alloc kind=0 bytes=5 id=6 watch_null=-1", "ok 1", "ev free kind=0 id=6", "state end live=0 recs=0"]


def test_each_kinds_free_serves_that_kinds_blocks(exes):
    # free_all of one block per kind: the backend aborts when a block meets another kind's free, so a clean exit with one
    # "free kind=k" per block of kind k is the property
    log = _runs(exes, "free_all")
    frees = _events(_between(log, "free_all", "second"))
    assert {ln for ln in frees} == {f"ev free kind={k} id={k + 1}" for k in range(5)}


@pytest.mark.parametrize("mode,words", [("backend_double_free", "unknown or already freed"), ("backend_wrong_kind", "freed by kind")])
def test_the_backend_guards_abort(exes, mode, words):
    done = subprocess.run([exes["plain"], mode], capture_output=True, text=True)
    assert done.returncode != 0 and "ABORT" in done.stdout and words in done.stdout
