"""The headers beside sdrhip.h (abi.SIDE_HEADERS), one test per registered header: binding one of them leaves sdrhip.h's
binding and every other side header's as they were, its names are its own, and its wrappers live in a module of their own,
not in nodes.py. What is particular to one header's module stays in that header's test file."""
import importlib

import pytest

import libsdr_amd  # noqa: F401   (the package imports every side header's module)
from libsdr_amd import abi, nodes

# side header -> (its binding module, the module of its wrappers)
MODULES = {"sdrhip_rx.h": ("abi_rx", "receiver"), "sdrhip_pocsag.h": ("abi_pocsag", "pocsag"), "sdrhip_agc.h": ("abi_agc", "agc"),
           "sdrhip_psk31.h": ("abi_psk31", "psk31")}


def test_every_registered_header_is_listed_here():
    assert sorted(abi.SIDE_HEADERS) == sorted(MODULES)


def _state(others):
    return dict(abi.SIGNATURES), list(abi.lib()._declared), {k: dict(v.SIGNATURES) for k, v in others.items()}


@pytest.mark.parametrize("header", sorted(MODULES))
def test_the_other_headers_bindings_are_unchanged_by_this_module(header):
    others = {k: v for k, v in abi.SIDE_HEADERS.items() if k != header}
    before = _state(others)
    wrappers = sorted(k for k, v in vars(nodes).items() if isinstance(v, type))
    binding = importlib.import_module("libsdr_amd." + MODULES[header][0])
    importlib.import_module("libsdr_amd." + MODULES[header][1])
    assert binding.SIGNATURES is abi.SIDE_HEADERS[header].SIGNATURES and binding.lib() is abi.lib()
    assert _state(others) == before
    assert sorted(abi.lib()._declared) == abi.header_functions()
    names = set(binding.header_functions())
    assert names
    for other in [abi.header_functions(), abi.SIGNATURES] + [t for v in others.values() for t in (v.header_functions(), v.SIGNATURES)]:
        assert not names & set(other)
    assert sorted(k for k, v in vars(nodes).items() if isinstance(v, type)) == wrappers
