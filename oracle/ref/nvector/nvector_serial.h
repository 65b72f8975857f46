/* Stand-in for SUNDIALS' nvector/nvector_serial.h, written for this repository (no SUNDIALS text).
 *
 * The reference model's units include this header through Macros.hpp, but outside the CVODE set-up they use
 * only the vector *container*: the N_Vector handle and the accessors NV_DATA_S / NV_Ith_S (f.cpp,
 * MD_update.cpp, MD_initialize.cpp).  This file declares exactly that container (length, ownership flag, data
 * pointer) so those units compile without SUNDIALS.  It holds no solver, no vector operations and no code. */
#ifndef SHUD_REF_STANDIN_NVECTOR_SERIAL_H
#define SHUD_REF_STANDIN_NVECTOR_SERIAL_H
struct _N_VectorContent_Serial { long length; int own_data; double *data; };
typedef struct _N_VectorContent_Serial *N_VectorContent_Serial;
struct _generic_N_Vector { void *content; };
typedef struct _generic_N_Vector *N_Vector;
#define NV_CONTENT_S(v) ((N_VectorContent_Serial)((v)->content))
#define NV_DATA_S(v) (NV_CONTENT_S(v)->data)
#define NV_Ith_S(v, i) (NV_DATA_S(v)[i])
#endif
