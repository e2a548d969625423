// The fp16- and bf16-map instances of pe_tab_kernel (pe_tab96.hip): the same source, instantiated for map_f16 / map_bf16 in this translation unit of
// their own, so that the fp32 instance's module -- and with it hipcc's register allocation of that kernel -- stays what it was (see pe_tab96.hip).
#define MV2D_PE_TAB_MAP16
#include "pe_tab96.hip"
