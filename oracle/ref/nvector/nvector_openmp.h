/* Stand-in for SUNDIALS' nvector/nvector_openmp.h (the -D_OPENMP_ON build of the reference), written for this
 * repository: the vector container and the accessors NV_DATA_OMP / NV_Ith_OMP only, as nvector_serial.h beside
 * it.  No SUNDIALS text, no vector operations, no code. */
#ifndef SHUD_REF_STANDIN_NVECTOR_OPENMP_H
#define SHUD_REF_STANDIN_NVECTOR_OPENMP_H
struct _N_VectorContent_OpenMP { long length; int own_data; double *data; int num_threads; };
typedef struct _N_VectorContent_OpenMP *N_VectorContent_OpenMP;
struct _generic_N_Vector { void *content; };
typedef struct _generic_N_Vector *N_Vector;
#define NV_CONTENT_OMP(v) ((N_VectorContent_OpenMP)((v)->content))
#define NV_DATA_OMP(v) (NV_CONTENT_OMP(v)->data)
#define NV_Ith_OMP(v, i) (NV_DATA_OMP(v)[i])
#endif
