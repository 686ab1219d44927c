"""The user table at the top of csrc/workspace.hpp against the ws_reserve call sites of csrc/: the header asks that the table be kept
in step with `grep ws_reserve`, and this is the grep."""
import os

import ws_ledger


def test_every_reserve_site_names_its_slot_literally():
    """A slot passed in a variable would hide the user from the ledger (and from a reader)."""
    slots = set(ws_ledger.slot_names())
    assert len(slots) == 18
    sites = ws_ledger.reserve_sites()
    assert len(sites) >= 30 and sum(len(v) for v in sites.values()) >= 70     # the grep found them: 38 pairs, 76 calls when written
    for (file, slot), lines in sites.items():
        assert slot in slots, f"{file}:{lines[0]}: ws_reserve of {slot!r}, not a WsSlot name"


def test_table_and_reserve_sites_name_the_same_file_slot_pairs():
    table = ws_ledger.table()
    assert sorted(table) == sorted(ws_ledger.slot_names()), "every slot has a row, and only slots have rows"
    stated = {(file, slot) for slot, files in table.items() for file in files}
    found = set(ws_ledger.reserve_sites())
    missing = sorted(found - stated)
    stale = sorted(stated - found)
    assert not missing, f"reserved in the code, missing from the table in workspace.hpp: {missing}"
    assert not stale, f"named in the table in workspace.hpp, but the file no longer reserves that slot: {stale}"


def test_table_names_functions_that_exist_in_their_file():
    """panel_plan.hpp reserves on behalf of its callers, which the table names after it: those live in other files of csrc/."""
    sources = {}
    for name in sorted(os.listdir(ws_ledger.CSRC)):
        if name.endswith((".hip", ".hpp")):
            with open(os.path.join(ws_ledger.CSRC, name)) as f:
                sources[name] = f.read()
    has = lambda src, fn: fn + "(" in src or fn + "<" in src                 # noqa: E731
    for slot, files in ws_ledger.table().items():
        for file, functions in files.items():
            assert functions, f"{slot}: {file} is named without a function"
            for fn in functions:
                if file == "panel_plan.hpp" and fn != "panel_query_block":
                    assert any(has(src, fn) for src in sources.values()), f"{slot}: no file of csrc/ has a function {fn}"
                else:
                    assert has(sources[file], fn), f"{slot}: {file} has no function {fn}"


def test_parser_reads_the_rows_it_is_known_to_hold():
    table = ws_ledger.table()
    assert table["WS_STAGE_IN"] == {"api.hip": ["pvs_vlad_encode", "pvs_fisher_encode", "pvs_cosine", "pvs_cosine_topk", "pvs_cosine_topk_f64"]}
    assert table["WS_SIFT_TABLES"] == table["WS_SIFT_PYRAMID"] == {"sift.hip": ["pvs_sift_dev"]}
    assert table["WS_PROJECTED"]["subset.hip"] == ["pvs_cosine_topk_subset_dev", "pvs_sq8_topk_subset_dev"]
    assert "launch_kmeans_step" in table["WS_SCRATCH"]["learn.hip"] and "pvs_ivf_sq8_group_probes_dev" in table["WS_UPDATE"]["ivf_sq8.hip"]
    assert ("WS_LISTS", "pvs_pair_components_dev") in ws_ledger.table_pairs()
