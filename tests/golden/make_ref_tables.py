"""Generate tests/golden/ref_tables.npz: the constant tables and the 12-bit ADC capture the reference ships, as data.

Run where the reference tree exists:   python tests/golden/make_ref_tables.py <reference root>

  hamm, tri_cen, tri_odd, tri_even, dct_arg   the tables of Src/Speech_Recog/MFCC_Arg.h:6-44 (values only)
  fft_table                                   the 2040 halfwords (Kr', Ki pairs) of TableFFT_V7, Src/BSP/cr4_fft_1024_stm32.s:285-629
  adc_stm32_123                               the 16 000 12-bit codes of Matlab/语音样本/STM32 123.txt

The tests compare the project's table generators and the oracle with these arrays, so they run without the reference.
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = ("hamm", "tri_cen", "tri_odd", "tri_even", "dct_arg")


def _text(root, rel):
    return open(os.path.join(root, rel), "rb").read().decode("latin1")


def header_tables(root):
    src = _text(root, "Src/Speech_Recog/MFCC_Arg.h")
    out = {}
    for name in TABLES:
        m = re.search(name + r"\[\]\s*=\s*\{([^}]*)\}", src)
        out[name] = np.array([int(v) for v in re.findall(r"-?\d+", m.group(1))], dtype=np.int64)
    return out


def asm_table(root):
    s = _text(root, "Src/BSP/cr4_fft_1024_stm32.s")
    tab = s[s.index("TableFFT_V7", s.index("passloop_v7")):]
    tab = tab[tab.index("\n"):]
    hw = [int(h, 16) for line in tab.splitlines() if "DCW" in line
          for h in re.findall(r"0x([0-9a-fA-F]{4})", line.split(";")[0])]
    return np.array(hw, dtype=np.uint16).view(np.int16)


def adc_dump(root):
    txt = open(os.path.join(root, "Matlab", "语音样本", "STM32 123.txt"), "rb").read().decode("latin1")
    return np.array([int(x) for x in re.findall(r"\d+", txt)], dtype=np.uint16)


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tests/golden/make_ref_tables.py <reference root>")
    root = sys.argv[1]
    g = header_tables(root)
    g["fft_table"] = asm_table(root)
    g["adc_stm32_123"] = adc_dump(root)
    assert len(g["fft_table"]) == 2040 and len(g["adc_stm32_123"]) == 16000
    np.savez_compressed(os.path.join(HERE, "ref_tables.npz"), **g)
    print({k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
