"""tests/caller_stream.py against the headers, without a GPU: the table has a row for exactly the exported functions that take a
stream, every sentence a row quotes stands in that function's header comment, and the parser the two checks rest on finds a new
declaration and misses none (tried on a scratch copy of a header)."""
import os
import re
import shutil

import pytest

import caller_stream as CS


def test_table_rows_are_the_functions_that_take_a_stream():
    """A new entry point with a `void *stream` and no row fails here, and so does a row whose function is gone."""
    takers = CS.stream_takers()
    assert len(takers) == len(set(takers)) >= 43
    missing, stale = sorted(set(takers) - set(CS.TABLE)), sorted(set(CS.TABLE) - set(takers))
    assert not missing, "functions that take a stream and have no row in tests/caller_stream.py: %s" % missing
    assert not stale, "rows of tests/caller_stream.py that name no function with a stream parameter: %s" % stale


def test_rows_are_well_formed():
    for name, row in CS.TABLE.items():
        assert row["class"] in (CS.QUEUED, CS.BLOCKS, CS.STEP), name
        assert set(row) <= {"class", "via", "says", "blocks_when"}, name
        assert ("via" in row) == (row["class"] == CS.QUEUED), name
        assert ("says" in row) == (row["class"] == CS.BLOCKS), name
        assert "blocks_when" not in row or row["class"] == CS.QUEUED, name
    # the step family is the six step calls and nothing else
    assert CS.rows(CS.STEP) == sorted(n for n in CS.TABLE if re.match(r"rem2d_(world|worlds|groups)_step(_ex)?$", n)), CS.rows(CS.STEP)


@pytest.mark.parametrize("name", sorted(n for n in CS.TABLE if CS.quoted(n)))
def test_quoted_sentence_stands_in_the_header(name):
    """what a row says about blocking is what the header says about it, word for word"""
    header, _, comment = CS.declared()[name]
    for sentence in CS.quoted(name):
        assert " ".join(sentence.split()) in comment, "%s: include/%s does not say %r" % (name, header, sentence)


# -------------------------------------------------------------------------------------------------- the parser, on a scratch copy
def _scratch_headers(tmp_path):
    dst = tmp_path / "include"
    shutil.copytree(os.path.join(CS.ROOT, "include"), str(dst))
    return str(dst)


def test_parser_finds_a_new_stream_taker(tmp_path):
    inc = _scratch_headers(tmp_path)
    assert CS.stream_takers(inc) == CS.stream_takers()
    with open(os.path.join(inc, "rem2d_gather.h"), "a") as f:
        f.write("\n/* a new one */\nint rem2d_x(void *stream);\nint rem2d_y(int32_t n,\n            void  * stream );\nint rem2d_z(void *streams);\n")
    assert sorted(set(CS.stream_takers(inc)) - set(CS.stream_takers())) == ["rem2d_x", "rem2d_y"]
    assert CS.declared(inc)["rem2d_x"][2] == "a new one"


def test_parser_reads_what_the_step_group_struct_is_not():
    """`void *stream;` inside rem2d_step_group is a field, no function; a commented-out declaration is none either"""
    d = CS.declared()
    assert "rem2d_step_group" not in d and "rem2d_world_field" in d
    assert "rem2d_world_field" not in CS.stream_takers()
    assert "(a synchronising copy on `stream`)" in d["rem2d_world_render"][2]
