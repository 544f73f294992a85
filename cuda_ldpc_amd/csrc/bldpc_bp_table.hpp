// bldpc_bp_table.hpp -- the correction table of the sum-product decoder (bldpc_decode_layered_bp, include/bldpc.h):
// T[k] = the fp32 nearest to log1p(exp(-(k + 0.5) / 16)), k = 0 .. 127, the midpoints of 128 cells of width 1/16 over [0, 8).
// Literals, not a computation at run time: host, device and every machine carry the same bits (bldpc_bp_table exports them,
// tests/test_bp_cpu.py holds them within 1 ulp of numpy's log1p(exp(.))).  Hexadecimal floats, so no decimal rounding either.
#pragma once

#define BLDPC_BP_TABLE_VALUES \
    0x1.5af430p-1f, 0x1.4b7422p-1f, 0x1.3c73c8p-1f, 0x1.2df2a2p-1f, 0x1.1feff0p-1f, 0x1.126abap-1f, 0x1.0561ccp-1f, 0x1.f1a768p-2f, \
    0x1.d97da0p-2f, 0x1.c24292p-2f, 0x1.abf230p-2f, 0x1.968814p-2f, 0x1.81ff88p-2f, 0x1.6e538ep-2f, 0x1.5b7eeap-2f, 0x1.497c20p-2f, \
    0x1.38458cp-2f, 0x1.27d55ep-2f, 0x1.1825a4p-2f, 0x1.093058p-2f, 0x1.f5debcp-3f, 0x1.dab926p-3f, 0x1.c0e3a0p-3f, 0x1.a851dcp-3f, \
    0x1.90f7a2p-3f, 0x1.7ac8d4p-3f, 0x1.65b976p-3f, 0x1.51bdbcp-3f, 0x1.3eca0cp-3f, 0x1.2cd30cp-3f, 0x1.1bcda0p-3f, 0x1.0baef2p-3f, \
    0x1.f8d8f4p-4f, 0x1.dbf7f8p-4f, 0x1.c0a718p-4f, 0x1.a6d324p-4f, 0x1.8e6994p-4f, 0x1.775886p-4f, 0x1.618ec8p-4f, 0x1.4cfbd0p-4f, \
    0x1.398fbep-4f, 0x1.273b54p-4f, 0x1.15f002p-4f, 0x1.059fd4p-4f, 0x1.ec7aecp-5f, 0x1.cf785cp-5f, 0x1.b41fb8p-5f, 0x1.9a59dep-5f, \
    0x1.8210cap-5f, 0x1.6b2f8cp-5f, 0x1.55a23cp-5f, 0x1.4155f2p-5f, 0x1.2e38bap-5f, 0x1.1c398cp-5f, 0x1.0b4844p-5f, 0x1.f6ab28p-6f, \
    0x1.d8a5fep-6f, 0x1.bc6598p-6f, 0x1.a1d002p-6f, 0x1.88ccacp-6f, 0x1.714460p-6f, 0x1.5b2130p-6f, 0x1.464e5ep-6f, 0x1.32b858p-6f, \
    0x1.204ca4p-6f, 0x1.0ef9d0p-6f, 0x1.fd5eccp-7f, 0x1.debbc2p-7f, 0x1.c1ed38p-7f, 0x1.a6d790p-7f, 0x1.8d60c8p-7f, 0x1.757054p-7f, \
    0x1.5eef1ap-7f, 0x1.49c752p-7f, 0x1.35e47ap-7f, 0x1.233342p-7f, 0x1.11a178p-7f, 0x1.011dfep-7f, 0x1.e33168p-8f, 0x1.c604dcp-8f, \
    0x1.aa99c6p-8f, 0x1.90d548p-8f, 0x1.789e16p-8f, 0x1.61dc64p-8f, 0x1.4c79d2p-8f, 0x1.38614ep-8f, 0x1.257f0ap-8f, 0x1.13c066p-8f, \
    0x1.0313dep-8f, 0x1.e6d1eap-9f, 0x1.c96060p-9f, 0x1.adb5f6p-9f, 0x1.93b74ap-9f, 0x1.7b4a9ap-9f, 0x1.6457b0p-9f, 0x1.4ec7c6p-9f, \
    0x1.3a8578p-9f, 0x1.277ca8p-9f, 0x1.159a6ep-9f, 0x1.04cd04p-9f, 0x1.ea0768p-10f, 0x1.cc5d9ap-10f, 0x1.b07f1ap-10f, 0x1.96502ap-10f, \
    0x1.7db6bcp-10f, 0x1.669a4cp-10f, 0x1.50e3dap-10f, 0x1.3c7dc2p-10f, 0x1.2953aep-10f, 0x1.175284p-10f, 0x1.066854p-10f, 0x1.ed0876p-11f, \
    0x1.cf2cc4p-11f, 0x1.b31fcap-11f, 0x1.98c588p-11f, 0x1.8003b4p-11f, 0x1.68c196p-11f, 0x1.52e7fap-11f, 0x1.3e610cp-11f, 0x1.2b1850p-11f, \
    0x1.18fa84p-11f, 0x1.07f590p-11f, 0x1.eff0eap-12f, 0x1.d1e674p-12f, 0x1.b5adbap-12f, 0x1.9b2a8cp-12f, 0x1.82426ep-12f, 0x1.6adc7cp-12f

namespace cldpc {

constexpr int kBpTableSize = 128;
constexpr float kBpTable[kBpTableSize] = {BLDPC_BP_TABLE_VALUES};

} // namespace cldpc
