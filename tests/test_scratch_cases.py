"""CPU: tests/scratch_cases.py imports without a GPU, its sharing table names only users and arenas that exist, and the arena table of
csrc/ctx.hip (what pvf_debug_scratch reports and fills) covers every DevBuf of the context."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyannote-video_amd", "csrc")


def _arena_table():
    """[(name, call_local)] of arena_table() in ctx.hip"""
    src = open(os.path.join(CSRC, "ctx.hip")).read()
    body = src[src.index("std::vector<ArenaRow> arena_table"):src.index("extern \"C\" int32_t pvf_debug_scratch")]
    return [(m.group(1), m.group(3) == "true") for m in re.finditer(r'\{"([a-z_0-9\[\]]+)", &c->([a-z_0-9\[\]]+), (true|false)\}', body)]


def test_the_sharing_table_names_users_and_arenas_that_exist():
    from tests import scratch_cases as sc
    arenas = dict(_arena_table())
    assert set(sc.SHARERS) <= set(arenas)
    assert set(u for users in sc.SHARERS.values() for u in users) == set(sc.USERS)
    for name, u in sc.USERS.items():
        assert u.name == name and callable(sc.step(name, "small")) and callable(sc.step(name, "large")) and sc.arenas_of(name)
        assert u.kind in (None, "landmarks", "embedder") and isinstance(u.rounds, dict)
    assert [a for a in sc.SHARERS if not arenas[a]] == ["s_orb_set"]          # the one listed arena that holds state
    for group in sc.SHARED:
        assert all(len(sc.SHARERS[a]) >= 2 and sc.SHARERS[a] == sc.SHARERS[group[0]] for a in group)
    assert sorted(a for g in sc.SHARED for a in g) == sorted(a for a, users in sc.SHARERS.items() if len(users) >= 2)


def test_the_arena_table_covers_every_device_buffer_of_the_context():
    hdr = open(os.path.join(CSRC, "pvf_internal.h")).read()
    ctx = hdr[hdr.index("struct Ctx {"):hdr.index("struct ProfScope")]
    declared = []
    for m in re.finditer(r"^    DevBuf ([^;]+);", ctx, re.M):
        for item in m.group(1).split(","):
            name, _, count = item.strip().partition("[")
            declared += [name] if not count else ["%s[%d]" % (name, k) for k in range(int(count.rstrip("]")))]
    table = _arena_table()
    assert len(declared) >= 28 and sorted(declared) == sorted(n for n, _ in table)
    assert [n for n, local in table if not local] == ["s_feat", "s_orb_set"]
