"""What include/vp_hip.h declares and what libvp_hip.so exports, for the "declared / exported / bound" tests."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vp_hip.h")


def header_source():
    """the header's text without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared_symbols():
    """names of the functions the header declares"""
    return set(re.findall(r"\b(vp_[a-z0-9_]+)\s*\(", header_source()))


def exported_symbols():
    """every defined dynamic symbol of the shipped library, of any type"""
    from autoware_vision_pilot_amd import lib

    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1].split("@")[0] for line in nm.splitlines() if line.strip()}
