"""starway_amd/_core.pyi names exactly what the native module holds.

The stub is written by hand, so a binding added without its stub entry (or
the reverse) shows here. Names only: module level without dunders, and the
public members of the classes that have any.
"""
import ast
from pathlib import Path

import pytest

from starway_amd import _core

TYPE_ALIASES = {"Buffer", "Index", "_Plan"}
CLASSES = ("Server", "Client", "ServerEndpoint", "_InboxRing")


def _dunder(name):
    return name.startswith("__") and name.endswith("__")


def _defined(body):
    """Names a module or class body defines (imports are not definitions)."""
    names = set()
    for node in body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.add(node.name)
        elif isinstance(node, ast.AnnAssign):
            names.add(node.target.id)
        elif isinstance(node, ast.Assign):
            names.update(t.id for t in node.targets)
    return names


@pytest.fixture(scope="module")
def stub():
    path = Path(_core.__file__).with_name("_core.pyi")
    return ast.parse(path.read_text()).body


def test_module_names_match_stub(stub):
    declared = {n for n in _defined(stub) if not _dunder(n)} - TYPE_ALIASES
    bound = {n for n in vars(_core) if not _dunder(n)}
    assert bound == declared


@pytest.mark.parametrize("cls", CLASSES)
def test_public_members_match_stub(stub, cls):
    node = next(n for n in stub
                if isinstance(n, ast.ClassDef) and n.name == cls)
    declared = {n for n in _defined(node.body) if not n.startswith("_")}
    bound = {n for n in vars(getattr(_core, cls)) if not n.startswith("_")}
    assert bound == declared
