!  lbfgsb_module -- the reference's public Fortran interface over the MI355X library.
!
!  Same module name, same public symbols (`setulb`, `lbfgsp_wp`) and the same
!  argument list as jacobwilliams/lbfgsb src/lbfgsb.f90:39-58, 88-89, so that the
!  reference's test/driver1.f90, driver2.f90 and driver3.f90 compile and link
!  unchanged.  Nothing is computed here: the call is forwarded through
!  iso_c_binding to `lbfgsb_hip_setulb_host_ik` (include/lbfgsb_hip.h), which runs
!  the iteration on the GPU.  Only the Fortran-specific marshalling lives here:
!  character(len=60) <-> char[60], logical <-> integer, optional file name.
!
!  Integer width: the module compiles unchanged with and without -fdefault-integer-8
!  (the build BASELINE.md section 3 calls mandatory at n = 1e8, src/lbfgsb.f90:246-265):
!  the width of the default INTEGER kind is handed to the library with every call.
!
!  -DREAL32 selects single precision exactly like the reference's
!  lbfgsb_kinds_module.F90:29-37 (REAL128 is not supported on the GPU).
      module lbfgsb_module

      use iso_c_binding
      use iso_fortran_env, only: output_unit, real32, real64

      implicit none

      private

#ifdef REAL32
      integer,parameter :: wp = real32
#else
      integer,parameter :: wp = real64
#endif
      integer,parameter,public :: lbfgsp_wp = wp

      public :: setulb
      ! Extensions beside the unchanged setulb: the DEVICE-POINTER forms of include/lbfgsb_hip.h for a Fortran
      ! caller whose x, l, u, nbd, g live in HBM (type(c_ptr) from hipMalloc through iso_c_binding) and whose
      ! objective runs on the GPU -- nothing n-long crosses PCIe.  Same reverse-communication protocol, same task
      ! strings, same isave / dsave / lsave slots as setulb (src/lbfgsb.f90:88-244); the work arrays wa / iwa are
      ! replaced by a context handle (examples/driver_dev.f90 is driver2's loop, test/driver2.f90:66-195, on them).
      public :: lbfgsb_create, lbfgsb_destroy          ! context of n rows, m pairs (lbfgsb_hip_create / _destroy)
      public :: setulb_dev                             ! lbfgsb_hip_setulb_dev: x, g updated in place on the device
      public :: setulb_dev_pp                          ! lbfgsb_hip_setulb_dev_pp: ping-pong iterate buffers
      public :: lbfgsb_objective                       ! built-in device objectives (lbfgsb_hip_objective)
      public :: lbfgsb_set_option                      ! per-context switches (lbfgsb_hip_set_option): 'compact_w', ...
      public :: lbfgsb_error_message                   ! text of the last failure (lbfgsb_hip_last_error)
      public :: lbfgsb_qn_apply, lbfgsb_qn_diag        ! the curvature model B, H = B^-1 of the last return on the
                                                       ! device (lbfgsb_hip_qn_apply / lbfgsb_hip_qn_diag)
      integer,parameter,public :: LBFGSB_QN_B = 0, LBFGSB_QN_H = 1
      integer,parameter,public :: LBFGSB_QN_B_SQRT = 4, LBFGSB_QN_H_SQRT = 5   ! lbfgsb_qn_apply only: A^(1/2) v
      public :: lbfgsb_qn_logdet, lbfgsb_qn_draw       ! log det A and draws mean + scale A^(1/2) z, z ~ N(0, I)
      public :: lbfgsb_qn_quad, lbfgsb_qn_logpdf, lbfgsb_qn_draw_logpdf   ! d'A d and Gaussian log-densities
      public :: lbfgsb_qn_gram                          ! the k x k matrix (V - center)' A (V - center)
      public :: lbfgsb_qn_eig, lbfgsb_qn_eigvec         ! eigenvalues and unit eigenvectors of B or H
      public :: lbfgsb_qn_shift_set, lbfgsb_qn_shift_solve, lbfgsb_qn_shift_logdet, lbfgsb_qn_shift_diag
      public :: lbfgsb_qn_shift_sqrt, lbfgsb_qn_shift_draw, lbfgsb_qn_shift_draw_logpdf   ! its factor and draws
      public :: lbfgsb_qn_shift_quad, lbfgsb_qn_shift_logpdf                              ! ... and densities
      public :: lbfgsb_qn_path_set, lbfgsb_qn_path_logdet, lbfgsb_qn_path_solve, lbfgsb_qn_path_trust  ! ... over a
      integer,parameter,public :: LBFGSB_QN_PATH_MAXK = 64                                            ! range of shifts
      public :: lbfgsb_qn_rows, lbfgsb_qn_block, lbfgsb_qn_cols       ! entries of B, H at lists of global 0-based rows
      public :: lbfgsb_qn_shift_block, lbfgsb_qn_shift_cols           ! ... and of (B + mu I + diag(d))^-1
      public :: lbfgsb_qn_pairs_get, lbfgsb_qn_pairs_set, lbfgsb_qn_pairs_push  ! the stored pairs as device data
      integer,parameter,public :: LBFGSB_QN_IDX_MAXK = 4096
                                                       ! solves, log det and diagonal of (B + mu I + diag(d))^-1
      public :: lbfgsb_kkt, lbfgsb_kkt_list            ! the active set, the bound multipliers and the projected
                                                       ! gradient of device arrays (lbfgsb_hip_kkt / _kkt_list)
      ! slots of lbfgsb_kkt's cnt(:) and val(:): the header's LBFGSB_KKT_* indices + 1 (Fortran arrays start at 1)
      integer,parameter,public :: LBFGSB_KKT_NCNT = 9, LBFGSB_KKT_NVAL = 4
      integer,parameter,public :: LBFGSB_KKT_N_UNBOUNDED = 1, LBFGSB_KKT_N_FREE = 2, LBFGSB_KKT_N_LOWER = 3,       &
                                  LBFGSB_KKT_N_UPPER = 4, LBFGSB_KKT_N_FIXED = 5, LBFGSB_KKT_N_BINDING = 6,        &
                                  LBFGSB_KKT_N_WEAK = 7, LBFGSB_KKT_N_LEAVING = 8, LBFGSB_KKT_N_OUTSIDE = 9
      integer,parameter,public :: LBFGSB_KKT_PG_MAX = 1, LBFGSB_KKT_MULT_MAX = 2, LBFGSB_KKT_OUT_MAX = 3,          &
                                  LBFGSB_KKT_GFREE_MAX = 4
      ! flags of lbfgsb_create (include/lbfgsb_hip.h)
      integer,parameter,public :: LBFGSB_F_REAL32 = 1, LBFGSB_F_MIRROR_INDEX = 2, LBFGSB_F_NO_RETURN_SYNC = 4, &
                                  LBFGSB_F_PARALLEL_GCP = 8, LBFGSB_F_INDEX_TIES = 32, LBFGSB_F_DEFER_LNSRCH = 64
      public :: lbfgsb_release   ! extension: frees the GPU context of a run that was stopped
                                 ! by the caller (task = 'STOP...' without another setulb call,
                                 ! as test/driver2.f90:174-195 does); harmless otherwise

      ! default INTEGER / LOGICAL width of THIS compilation (4, or 8 under -fdefault-integer-8): the
      ! library takes nbd, iwa, lsave, isave as arrays of that width (lbfgsb_hip_setulb_host_ik), so
      ! the same source serves both builds
      integer,parameter :: ibytes = storage_size(1)/8

      interface
         function lbfgsb_hip_setulb_host_ik(n,m,x,l,u,nbd,f,g,factr,pgtol,wa,iwa,task,iprint,  &
                                            csave,lsave,isave,dsave,iteration_file,real_bytes, &
                                            mirror,int_bytes)                                  &
                                            bind(C,name='lbfgsb_hip_setulb_host_ik') result(rc)
            import :: c_int32_t, c_int64_t, c_double, c_char, c_ptr, wp
            integer(c_int64_t),value :: n, m, iprint
            integer(c_int32_t),value :: real_bytes, mirror, int_bytes
            real(wp) :: x(*), l(*), u(*), g(*), wa(*), dsave(*)
            real(wp) :: f
            real(c_double),value :: factr, pgtol
            integer :: nbd(*), iwa(*), lsave(*), isave(*)   ! default kind: int_bytes wide
            character(kind=c_char) :: task(*), csave(*)
            type(c_ptr),value :: iteration_file
            integer(c_int32_t) :: rc
         end function lbfgsb_hip_setulb_host_ik
         function lbfgsb_hip_release_host_ik(isave,int_bytes)                                  &
                                             bind(C,name='lbfgsb_hip_release_host_ik') result(rc)
            import :: c_int32_t
            integer :: isave(*)
            integer(c_int32_t),value :: int_bytes
            integer(c_int32_t) :: rc
         end function lbfgsb_hip_release_host_ik
         function lbfgsb_hip_last_error() bind(C,name='lbfgsb_hip_last_error') result(p)
            import :: c_ptr
            type(c_ptr) :: p
         end function lbfgsb_hip_last_error
         ! ---- device-pointer forms (include/lbfgsb_hip.h) ----
         function lbfgsb_hip_create(n_local,n_global,row0,m,flags,device,stream,ctx)             &
                                    bind(C,name='lbfgsb_hip_create') result(rc)
            import :: c_int, c_int64_t, c_ptr
            integer(c_int64_t),value :: n_local, n_global, row0
            integer(c_int),value :: m, flags, device
            type(c_ptr),value :: stream
            type(c_ptr) :: ctx
            integer(c_int) :: rc
         end function lbfgsb_hip_create
         subroutine lbfgsb_hip_destroy(ctx) bind(C,name='lbfgsb_hip_destroy')
            import :: c_ptr
            type(c_ptr),value :: ctx
         end subroutine lbfgsb_hip_destroy
         function lbfgsb_hip_setulb_dev(ctx,x,l,u,nbd,f,g,factr,pgtol,task,iprint,csave,lsave,isave,dsave) &
                                        bind(C,name='lbfgsb_hip_setulb_dev') result(rc)
            import :: c_int, c_int32_t, c_double, c_char, c_ptr
            type(c_ptr),value :: ctx, x, l, u, nbd, g
            real(c_double) :: f, dsave(29)
            real(c_double),value :: factr, pgtol
            character(kind=c_char) :: task(*), csave(*)
            integer(c_int),value :: iprint
            integer(c_int32_t) :: lsave(4), isave(44)
            integer(c_int) :: rc
         end function lbfgsb_hip_setulb_dev
         function lbfgsb_hip_setulb_dev_pp(ctx,x0,x1,l,u,nbd,f,g0,g1,factr,pgtol,task,iprint,csave,lsave, &
                                           isave,dsave,cur) bind(C,name='lbfgsb_hip_setulb_dev_pp') result(rc)
            import :: c_int, c_int32_t, c_double, c_char, c_ptr
            type(c_ptr),value :: ctx, x0, x1, l, u, nbd, g0, g1
            real(c_double) :: f, dsave(29)
            real(c_double),value :: factr, pgtol
            character(kind=c_char) :: task(*), csave(*)
            integer(c_int),value :: iprint
            integer(c_int32_t) :: lsave(4), isave(44), cur
            integer(c_int) :: rc
         end function lbfgsb_hip_setulb_dev_pp
         function lbfgsb_hip_objective(ctx,kind,x,g,h_f) bind(C,name='lbfgsb_hip_objective') result(rc)
            import :: c_int, c_ptr
            type(c_ptr),value :: ctx, x, g, h_f
            integer(c_int),value :: kind
            integer(c_int) :: rc
         end function lbfgsb_hip_objective
         function lbfgsb_hip_set_option(ctx,name,val) bind(C,name='lbfgsb_hip_set_option') result(rc)
            import :: c_int, c_ptr, c_char, c_double
            type(c_ptr),value :: ctx
            character(kind=c_char) :: name(*)
            real(c_double),value :: val
            integer(c_int) :: rc
         end function lbfgsb_hip_set_option
         function lbfgsb_hip_qn_apply(ctx,mode,k,v,ldv,out,ldo) bind(C,name='lbfgsb_hip_qn_apply') result(rc)
            import :: c_int, c_int64_t, c_ptr
            type(c_ptr),value :: ctx, v, out
            integer(c_int),value :: mode
            integer(c_int64_t),value :: k, ldv, ldo
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_apply
         function lbfgsb_hip_qn_diag(ctx,mode,out) bind(C,name='lbfgsb_hip_qn_diag') result(rc)
            import :: c_int, c_ptr
            type(c_ptr),value :: ctx, out
            integer(c_int),value :: mode
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_diag
         function lbfgsb_hip_qn_logdet(ctx,mode,logdet) bind(C,name='lbfgsb_hip_qn_logdet') result(rc)
            import :: c_int, c_double, c_ptr
            type(c_ptr),value :: ctx
            integer(c_int),value :: mode
            real(c_double) :: logdet
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_logdet
         function lbfgsb_hip_qn_shift_set(ctx,d,mu,pinned) bind(C,name='lbfgsb_hip_qn_shift_set') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, d
            real(c_double),value :: mu
            integer(c_int64_t) :: pinned
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_set
         function lbfgsb_hip_qn_shift_solve(ctx,k,v,ldv,out,ldo) bind(C,name='lbfgsb_hip_qn_shift_solve') result(rc)
            import :: c_int, c_int64_t, c_ptr
            type(c_ptr),value :: ctx, v, out
            integer(c_int64_t),value :: k, ldv, ldo
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_solve
         function lbfgsb_hip_qn_shift_logdet(ctx,logdet) bind(C,name='lbfgsb_hip_qn_shift_logdet') result(rc)
            import :: c_int, c_double, c_ptr
            type(c_ptr),value :: ctx
            real(c_double) :: logdet
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_logdet
         function lbfgsb_hip_qn_path_set(ctx,status,code_mask,pinned) bind(C,name='lbfgsb_hip_qn_path_set') result(rc)
            import :: c_int, c_int64_t, c_ptr
            type(c_ptr),value :: ctx, status
            integer(c_int),value :: code_mask
            integer(c_int64_t) :: pinned
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_path_set
         function lbfgsb_hip_qn_path_logdet(ctx,k,mu,logdet,info) bind(C,name='lbfgsb_hip_qn_path_logdet') result(rc)
            import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx
            integer(c_int64_t),value :: k
            real(c_double) :: mu(*), logdet(*)
            integer(c_int32_t) :: info(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_path_logdet
         function lbfgsb_hip_qn_path_solve(ctx,v,k,mu,out,ldo,norm2,vx) bind(C,name='lbfgsb_hip_qn_path_solve')    &
            result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, v, out
            integer(c_int64_t),value :: k, ldo
            real(c_double) :: mu(*), norm2(*), vx(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_path_solve
         function lbfgsb_hip_qn_path_trust(ctx,g,delta,rtol,max_it,step,res,iters)                                 &
            bind(C,name='lbfgsb_hip_qn_path_trust') result(rc)
            import :: c_int, c_int32_t, c_double, c_ptr
            type(c_ptr),value :: ctx, g, step
            real(c_double),value :: delta, rtol
            integer(c_int),value :: max_it
            real(c_double) :: res(4)
            integer(c_int32_t) :: iters
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_path_trust
         function lbfgsb_hip_qn_shift_diag(ctx,out) bind(C,name='lbfgsb_hip_qn_shift_diag') result(rc)
            import :: c_int, c_ptr
            type(c_ptr),value :: ctx, out
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_diag
         function lbfgsb_hip_qn_shift_sqrt(ctx,k,v,ldv,out,ldo) bind(C,name='lbfgsb_hip_qn_shift_sqrt') result(rc)
            import :: c_int, c_int64_t, c_ptr
            type(c_ptr),value :: ctx, v, out
            integer(c_int64_t),value :: k, ldv, ldo
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_sqrt
         function lbfgsb_hip_qn_shift_draw(ctx,k,seed,first,mean,scale,out,ldo) &
            bind(C,name='lbfgsb_hip_qn_shift_draw') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, mean, out
            integer(c_int64_t),value :: k, seed, first, ldo
            real(c_double),value :: scale
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_draw
         function lbfgsb_hip_qn_shift_draw_logpdf(ctx,k,seed,first,mean,scale,out,ldo,logp) &
            bind(C,name='lbfgsb_hip_qn_shift_draw_logpdf') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, mean, out
            integer(c_int64_t),value :: k, seed, first, ldo
            real(c_double),value :: scale
            real(c_double) :: logp(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_draw_logpdf
         function lbfgsb_hip_qn_shift_quad(ctx,k,v,ldv,center,q) bind(C,name='lbfgsb_hip_qn_shift_quad') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, v, center
            integer(c_int64_t),value :: k, ldv
            real(c_double) :: q(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_quad
         function lbfgsb_hip_qn_shift_logpdf(ctx,k,x,ldx,mean,scale,logp) bind(C,name='lbfgsb_hip_qn_shift_logpdf') &
            result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, x, mean
            integer(c_int64_t),value :: k, ldx
            real(c_double),value :: scale
            real(c_double) :: logp(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_logpdf
         function lbfgsb_hip_qn_draw(ctx,mode,k,seed,first,mean,scale,out,ldo) bind(C,name='lbfgsb_hip_qn_draw') &
            result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, mean, out
            integer(c_int),value :: mode
            integer(c_int64_t),value :: k, seed, first, ldo
            real(c_double),value :: scale
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_draw
         function lbfgsb_hip_qn_quad(ctx,mode,k,v,ldv,center,q) bind(C,name='lbfgsb_hip_qn_quad') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, v, center
            integer(c_int),value :: mode
            integer(c_int64_t),value :: k, ldv
            real(c_double) :: q(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_quad
         function lbfgsb_hip_qn_gram(ctx,mode,k,v,ldv,center,g,ldg) bind(C,name='lbfgsb_hip_qn_gram') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, v, center
            integer(c_int),value :: mode
            integer(c_int64_t),value :: k, ldv, ldg
            real(c_double) :: g(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_gram
         function lbfgsb_hip_qn_eig(ctx,mode,cap,r,bulk,lambda) bind(C,name='lbfgsb_hip_qn_eig') result(rc)
            import :: c_int, c_int32_t, c_double, c_ptr
            type(c_ptr),value :: ctx
            integer(c_int),value :: mode
            integer(c_int32_t),value :: cap
            integer(c_int32_t) :: r
            real(c_double) :: bulk
            real(c_double) :: lambda(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_eig
         function lbfgsb_hip_qn_eigvec(ctx,mode,k,which,out,ldo) bind(C,name='lbfgsb_hip_qn_eigvec') result(rc)
            import :: c_int, c_int32_t, c_int64_t, c_ptr
            type(c_ptr),value :: ctx, out
            integer(c_int),value :: mode
            integer(c_int64_t),value :: k, ldo
            integer(c_int32_t) :: which(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_eigvec
         function lbfgsb_hip_qn_logpdf(ctx,mode,k,x,ldx,mean,scale,logp) bind(C,name='lbfgsb_hip_qn_logpdf') &
            result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, x, mean
            integer(c_int),value :: mode
            integer(c_int64_t),value :: k, ldx
            real(c_double),value :: scale
            real(c_double) :: logp(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_logpdf
         function lbfgsb_hip_qn_draw_logpdf(ctx,mode,k,seed,first,mean,scale,out,ldo,logp) &
            bind(C,name='lbfgsb_hip_qn_draw_logpdf') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, mean, out
            integer(c_int),value :: mode
            integer(c_int64_t),value :: k, seed, first, ldo
            real(c_double),value :: scale
            real(c_double) :: logp(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_draw_logpdf
         function lbfgsb_hip_qn_rows(ctx,k,idx,rows,ldr) bind(C,name='lbfgsb_hip_qn_rows') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx
            integer(c_int64_t),value :: k, ldr
            integer(c_int64_t) :: idx(*)
            real(c_double) :: rows(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_rows
         function lbfgsb_hip_qn_block(ctx,mode,ka,ia,kb,ib,a,lda) bind(C,name='lbfgsb_hip_qn_block') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, ib
            integer(c_int),value :: mode
            integer(c_int64_t),value :: ka, kb, lda
            integer(c_int64_t) :: ia(*)
            real(c_double) :: a(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_block
         function lbfgsb_hip_qn_cols(ctx,mode,k,idx,out,ldo) bind(C,name='lbfgsb_hip_qn_cols') result(rc)
            import :: c_int, c_int64_t, c_ptr
            type(c_ptr),value :: ctx, out
            integer(c_int),value :: mode
            integer(c_int64_t),value :: k, ldo
            integer(c_int64_t) :: idx(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_cols
         function lbfgsb_hip_qn_shift_block(ctx,ka,ia,kb,ib,a,lda) bind(C,name='lbfgsb_hip_qn_shift_block') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, ib
            integer(c_int64_t),value :: ka, kb, lda
            integer(c_int64_t) :: ia(*)
            real(c_double) :: a(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_block
         function lbfgsb_hip_qn_shift_cols(ctx,k,idx,out,ldo) bind(C,name='lbfgsb_hip_qn_shift_cols') result(rc)
            import :: c_int, c_int64_t, c_ptr
            type(c_ptr),value :: ctx, out
            integer(c_int64_t),value :: k, ldo
            integer(c_int64_t) :: idx(*)
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_shift_cols
         function lbfgsb_hip_qn_pairs_get(ctx,cap,col,theta,s,lds,y,ldy) bind(C,name='lbfgsb_hip_qn_pairs_get') result(rc)
            import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, s, y
            integer(c_int32_t),value :: cap
            integer(c_int32_t) :: col
            real(c_double) :: theta
            integer(c_int64_t),value :: lds, ldy
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_pairs_get
         function lbfgsb_hip_qn_pairs_set(ctx,k,s,lds,y,ldy,theta) bind(C,name='lbfgsb_hip_qn_pairs_set') result(rc)
            import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, s, y
            integer(c_int32_t),value :: k
            integer(c_int64_t),value :: lds, ldy
            real(c_double),value :: theta
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_pairs_set
         function lbfgsb_hip_qn_pairs_push(ctx,s,y,theta,stored) bind(C,name='lbfgsb_hip_qn_pairs_push') result(rc)
            import :: c_int, c_int32_t, c_double, c_ptr
            type(c_ptr),value :: ctx, s, y
            real(c_double),value :: theta
            integer(c_int32_t) :: stored
            integer(c_int) :: rc
         end function lbfgsb_hip_qn_pairs_push
         function lbfgsb_hip_kkt(ctx,x,l,u,nbd,g,tol,pg,mult,status,cnt,val) bind(C,name='lbfgsb_hip_kkt') result(rc)
            import :: c_int, c_int64_t, c_double, c_ptr
            type(c_ptr),value :: ctx, x, l, u, nbd, g, pg, mult, status
            real(c_double),value :: tol
            integer(c_int64_t) :: cnt(9)
            real(c_double) :: val(4)
            integer(c_int) :: rc
         end function lbfgsb_hip_kkt
         function lbfgsb_hip_kkt_list(ctx,status,code_mask,idx,cap,count) bind(C,name='lbfgsb_hip_kkt_list') result(rc)
            import :: c_int, c_int64_t, c_ptr
            type(c_ptr),value :: ctx, status, idx
            integer(c_int),value :: code_mask
            integer(c_int64_t),value :: cap
            integer(c_int64_t) :: count
            integer(c_int) :: rc
         end function lbfgsb_hip_kkt_list
         function c_strlen(s) bind(C,name='strlen') result(k)
            import :: c_ptr, c_size_t
            type(c_ptr),value :: s
            integer(c_size_t) :: k
         end function c_strlen
      end interface

      contains

      subroutine setulb(n,m,x,l,u,Nbd,f,g,Factr,Pgtol,Wa,Iwa,Task, &
                        Iprint,Csave,Lsave,Isave,Dsave,iteration_file)

      integer,intent(in) :: n
      integer,intent(in) :: m
      real(wp),intent(inout) :: x(n)
      real(wp),intent(in) :: l(n)
      real(wp),intent(in) :: u(n)
      integer,intent(in) :: Nbd(n)
      real(wp),intent(inout) :: f
      real(wp),intent(inout) :: g(n)
      real(wp),intent(in) :: Factr
      real(wp),intent(in) :: Pgtol
      real(wp) :: Wa(*)
      integer :: Iwa(*)
      character(len=60),intent(inout) :: Task
      integer,intent(in) :: Iprint
      character(len=60) :: Csave
      logical :: Lsave(4)
      integer :: Isave(44)
      real(wp) :: Dsave(29)
      character(len=*),intent(in),optional :: iteration_file

      character(kind=c_char) :: ctask(60), ccsave(60)
      character(kind=c_char),allocatable,target :: cfile(:)
      integer :: clsave(4)
      integer(c_int32_t) :: rc
      type(c_ptr) :: pfile
      integer :: i, k

      do i = 1, 60
         ctask(i) = Task(i:i)
         ccsave(i) = Csave(i:i)
      end do
      do i = 1, 4
         clsave(i) = merge(1, 0, Lsave(i))
      end do
      pfile = c_null_ptr
      if (present(iteration_file)) then
         k = len_trim(iteration_file)
         allocate (cfile(k + 1))
         do i = 1, k
            cfile(i) = iteration_file(i:i)
         end do
         cfile(k + 1) = c_null_char
         pfile = c_loc(cfile)
      end if

      ! the library prints through C stdio: keep the two output streams in order
      if (Iprint >= 0) flush (output_unit)

      rc = lbfgsb_hip_setulb_host_ik(int(n, c_int64_t), int(m, c_int64_t), x, l, u, Nbd, f, g,        &
                                     real(Factr, c_double), real(Pgtol, c_double), Wa, Iwa, ctask,    &
                                     int(Iprint, c_int64_t), ccsave, clsave, Isave, Dsave, pfile,     &
                                     int(storage_size(1.0_wp)/8, c_int32_t), 0_c_int32_t,             &
                                     int(ibytes, c_int32_t))

      do i = 1, 60
         Task(i:i) = ctask(i)
         Csave(i:i) = ccsave(i)
      end do
      do i = 1, 4
         Lsave(i) = clsave(i) /= 0
      end do
      if (rc /= 0) then
         ! no GPU, no library, bad call sequence: there is no CPU path to fall back to
         write (output_unit,'(a,i0)') ' lbfgsb_hip_setulb_host failed, code ', rc
         Task = 'ERROR: LBFGSB_HIP FAILURE'
      end if

      end subroutine setulb

!  ---------------------------------------------------------------------------------------------------------
!  Device-pointer forms.  x, l, u, nbd, g are type(c_ptr) DEVICE addresses (real(wp) values, nbd 32-bit
!  integers, 16-byte aligned); f, task, csave, lsave, isave, dsave are ordinary host variables with setulb's
!  meaning slot for slot.  rc = 0, or the library's error code (text: lbfgsb_error_message()).
!  ---------------------------------------------------------------------------------------------------------

      subroutine lbfgsb_create(ctx, n, m, flags, rc, device)
      type(c_ptr),intent(out) :: ctx
      integer,intent(in) :: n, m
      integer,intent(in) :: flags            ! sum of LBFGSB_F_*; LBFGSB_F_REAL32 is added for a -DREAL32 build
      integer,intent(out) :: rc
      integer,intent(in),optional :: device
      integer(c_int) :: fl, dev
      fl = int(flags, c_int)
      if (storage_size(1.0_wp) == 32) fl = ior(fl, int(LBFGSB_F_REAL32, c_int))
      dev = 0
      if (present(device)) dev = int(device, c_int)
      ctx = c_null_ptr
      rc = lbfgsb_hip_create(int(n, c_int64_t), int(n, c_int64_t), 0_c_int64_t, int(m, c_int), fl, dev, &
                             c_null_ptr, ctx)
      end subroutine lbfgsb_create

      subroutine lbfgsb_destroy(ctx)
      type(c_ptr),intent(inout) :: ctx
      if (c_associated(ctx)) call lbfgsb_hip_destroy(ctx)
      ctx = c_null_ptr
      end subroutine lbfgsb_destroy

      subroutine marshal_in(Task, Csave, Lsave, Isave, Dsave, f, ctask, ccsave, l32, i32, d64, f64)
      character(len=60),intent(in) :: Task, Csave
      logical,intent(in) :: Lsave(4)
      integer,intent(in) :: Isave(44)
      real(wp),intent(in) :: Dsave(29), f
      character(kind=c_char),intent(out) :: ctask(60), ccsave(60)
      integer(c_int32_t),intent(out) :: l32(4), i32(44)
      real(c_double),intent(out) :: d64(29), f64
      integer :: i
      do i = 1, 60
         ctask(i) = Task(i:i)
         ccsave(i) = Csave(i:i)
      end do
      do i = 1, 4
         l32(i) = merge(1_c_int32_t, 0_c_int32_t, Lsave(i))
      end do
      i32 = int(Isave, c_int32_t)
      d64 = real(Dsave, c_double)
      f64 = real(f, c_double)
      end subroutine marshal_in

      subroutine marshal_out(Task, Csave, Lsave, Isave, Dsave, f, ctask, ccsave, l32, i32, d64, f64)
      character(len=60),intent(out) :: Task, Csave
      logical,intent(out) :: Lsave(4)
      integer,intent(out) :: Isave(44)
      real(wp),intent(out) :: Dsave(29), f
      character(kind=c_char),intent(in) :: ctask(60), ccsave(60)
      integer(c_int32_t),intent(in) :: l32(4), i32(44)
      real(c_double),intent(in) :: d64(29), f64
      integer :: i
      do i = 1, 60
         Task(i:i) = ctask(i)
         Csave(i:i) = ccsave(i)
      end do
      do i = 1, 4
         Lsave(i) = l32(i) /= 0
      end do
      Isave = int(i32, kind(Isave))
      Dsave = real(d64, wp)
      f = real(f64, wp)
      end subroutine marshal_out

      subroutine setulb_dev(ctx, x, l, u, Nbd, f, g, Factr, Pgtol, Task, Iprint, Csave, Lsave, Isave, Dsave, rc)
      type(c_ptr),intent(in) :: ctx
      type(c_ptr),intent(in) :: x, l, u, Nbd, g        ! device pointers
      real(wp),intent(inout) :: f
      real(wp),intent(in) :: Factr, Pgtol
      character(len=60),intent(inout) :: Task
      integer,intent(in) :: Iprint
      character(len=60) :: Csave
      logical :: Lsave(4)
      integer :: Isave(44)
      real(wp) :: Dsave(29)
      integer,intent(out) :: rc
      character(kind=c_char) :: ctask(60), ccsave(60)
      integer(c_int32_t) :: l32(4), i32(44)
      real(c_double) :: d64(29), f64
      call marshal_in(Task, Csave, Lsave, Isave, Dsave, f, ctask, ccsave, l32, i32, d64, f64)
      if (Iprint >= 0) flush (output_unit)
      rc = lbfgsb_hip_setulb_dev(ctx, x, l, u, Nbd, f64, g, real(Factr, c_double), real(Pgtol, c_double), ctask, &
                                 int(Iprint, c_int), ccsave, l32, i32, d64)
      call marshal_out(Task, Csave, Lsave, Isave, Dsave, f, ctask, ccsave, l32, i32, d64, f64)
      if (rc /= 0) Task = 'ERROR: LBFGSB_HIP FAILURE'
      end subroutine setulb_dev

      ! Ping-pong form: TWO buffers for x and two for g; cur (0 or 1) says which pair this return refers to --
      ! evaluate f at x(cur) into g(cur) on 'FG...', x(cur) / g(cur) are the iterate on 'NEW_X' and at the end
      ! (include/lbfgsb_hip.h: nothing is copied for t = x, r = g of src/lbfgsb.f90:2235-2236).
      subroutine setulb_dev_pp(ctx, x0, x1, l, u, Nbd, f, g0, g1, Factr, Pgtol, Task, Iprint, Csave, Lsave, Isave, &
                               Dsave, cur, rc)
      type(c_ptr),intent(in) :: ctx
      type(c_ptr),intent(in) :: x0, x1, l, u, Nbd, g0, g1     ! device pointers
      real(wp),intent(inout) :: f
      real(wp),intent(in) :: Factr, Pgtol
      character(len=60),intent(inout) :: Task
      integer,intent(in) :: Iprint
      character(len=60) :: Csave
      logical :: Lsave(4)
      integer :: Isave(44)
      real(wp) :: Dsave(29)
      integer,intent(out) :: cur, rc
      character(kind=c_char) :: ctask(60), ccsave(60)
      integer(c_int32_t) :: l32(4), i32(44), c32
      real(c_double) :: d64(29), f64
      call marshal_in(Task, Csave, Lsave, Isave, Dsave, f, ctask, ccsave, l32, i32, d64, f64)
      if (Iprint >= 0) flush (output_unit)
      c32 = 0
      rc = lbfgsb_hip_setulb_dev_pp(ctx, x0, x1, l, u, Nbd, f64, g0, g1, real(Factr, c_double),               &
                                    real(Pgtol, c_double), ctask, int(Iprint, c_int), ccsave, l32, i32, d64, c32)
      call marshal_out(Task, Csave, Lsave, Isave, Dsave, f, ctask, ccsave, l32, i32, d64, f64)
      cur = int(c32)
      if (rc /= 0) Task = 'ERROR: LBFGSB_HIP FAILURE'
      end subroutine setulb_dev_pp

      ! A switch of this context (include/lbfgsb_hip.h, lbfgsb_hip_set_option), before 'START': e.g.
      ! call lbfgsb_set_option(ctx, 'compact_w', 1.0d0, rc) -- the two passes over W read the W entries of the free
      ! variables only (the reference's Index(1:nfree) loops, src/lbfgsb.f90:1565-1583, 2743-2778; DESIGN.md 4g)
      subroutine lbfgsb_set_option(ctx, name, val, rc)
      type(c_ptr),intent(in) :: ctx
      character(len=*),intent(in) :: name
      real(c_double),intent(in) :: val
      integer,intent(out) :: rc
      character(kind=c_char) :: cname(len_trim(name) + 1)
      integer :: k
      do k = 1, len_trim(name)
         cname(k) = name(k:k)
      end do
      cname(len_trim(name) + 1) = c_null_char
      rc = lbfgsb_hip_set_option(ctx, cname, val)
      end subroutine lbfgsb_set_option

      ! Built-in objective on the context's stream: kind 0 = separable bounded quadratic (BASELINE.md 3),
      ! 1 = extended Rosenbrock (test/driver1.f90:274-289).  With f present the call waits for the value;
      ! without it the value stays on the device and the NEXT setulb_dev / setulb_dev_pp call (the 'FG' re-entry)
      ! brings it over with its own sums and stores it in its f argument: one host sync per evaluation less.
      subroutine lbfgsb_objective(ctx, kind, x, g, rc, f)
      type(c_ptr),intent(in) :: ctx, x, g
      integer,intent(in) :: kind
      integer,intent(out) :: rc
      real(wp),intent(out),optional :: f
      real(c_double),target :: f64
      if (present(f)) then
         rc = lbfgsb_hip_objective(ctx, int(kind, c_int), x, g, c_loc(f64))
         f = real(f64, wp)
      else
         rc = lbfgsb_hip_objective(ctx, int(kind, c_int), x, g, c_null_ptr)
      end if
      end subroutine lbfgsb_objective

      ! The curvature model of the last return (include/lbfgsb_hip.h, "The curvature model as a device operator"):
      ! mode LBFGSB_QN_B (B, bmv's matrix) or LBFGSB_QN_H (H = B^-1).  lbfgsb_qn_apply: out_j = A v_j for k vectors
      ! of the context's real kind, vector j at v + j*ldv elements, result j at out + j*ldo (device buffers,
      ! ldv, ldo >= n).  lbfgsb_qn_diag: out = diag(A), at most 32 stored pairs.  rc as the C entries return it.
      subroutine lbfgsb_qn_apply(ctx, mode, k, v, ldv, out, ldo, rc)
      type(c_ptr),intent(in) :: ctx, v, out
      integer,intent(in) :: mode, k, ldv, ldo
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_apply(ctx, int(mode, c_int), int(k, c_int64_t), v, int(ldv, c_int64_t), out, &
                               int(ldo, c_int64_t))
      end subroutine lbfgsb_qn_apply

      subroutine lbfgsb_qn_diag(ctx, mode, out, rc)
      type(c_ptr),intent(in) :: ctx, out
      integer,intent(in) :: mode
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_diag(ctx, int(mode, c_int), out)
      end subroutine lbfgsb_qn_diag

      ! The model plus a diagonal (include/lbfgsb_hip.h, "The model plus a diagonal"): (B + mu I + diag(d))^-1 on the
      ! rows that are not pinned.  lbfgsb_qn_shift_set: d is a device buffer of n reals of the context's kind or
      ! c_null_ptr (D = 0), an entry +inf pins its row; pinned receives the pinned rows of all ranks.  It makes the
      ! weights and the factor for the pairs of this return: after a return that stores a pair the other three return
      ! LBFGSB_E_STATE until it is called again.  lbfgsb_qn_shift_solve: out_j = (B + mu I + D)^-1 v_j, k vectors laid
      ! out as lbfgsb_qn_apply's, +0 on pinned rows.  lbfgsb_qn_shift_logdet: log det of the shifted model on the free
      ! rows.  lbfgsb_qn_shift_diag: the diagonal of the inverse (n reals), at most 32 stored pairs.
      subroutine lbfgsb_qn_shift_set(ctx, d, mu, pinned, rc)
      type(c_ptr),intent(in) :: ctx, d
      real(c_double),intent(in) :: mu
      integer(c_int64_t),intent(out) :: pinned
      integer,intent(out) :: rc
      pinned = 0
      rc = lbfgsb_hip_qn_shift_set(ctx, d, mu, pinned)
      end subroutine lbfgsb_qn_shift_set

      subroutine lbfgsb_qn_shift_solve(ctx, k, v, ldv, out, ldo, rc)
      type(c_ptr),intent(in) :: ctx, v, out
      integer,intent(in) :: k, ldv, ldo
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_solve(ctx, int(k, c_int64_t), v, int(ldv, c_int64_t), out, int(ldo, c_int64_t))
      end subroutine lbfgsb_qn_shift_solve

      subroutine lbfgsb_qn_shift_logdet(ctx, logdet, rc)
      type(c_ptr),intent(in) :: ctx
      real(c_double),intent(out) :: logdet
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_logdet(ctx, logdet)
      end subroutine lbfgsb_qn_shift_logdet

      subroutine lbfgsb_qn_shift_diag(ctx, out, rc)
      type(c_ptr),intent(in) :: ctx, out
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_diag(ctx, out)
      end subroutine lbfgsb_qn_shift_diag

      ! The model over a range of shifts (include/lbfgsb_hip.h, "The model over a range of shifts"): (B_FF + mu I)^-1 on
      ! the rows F that are not pinned, for any number of shifts after one lbfgsb_qn_path_set.  status: a device buffer
      ! of n int8 codes as lbfgsb_kkt writes them, or c_null_ptr (nothing pinned); bit (code + 1) of code_mask selects
      ! a code to PIN (28 = 0b11100: at a lower bound, at an upper bound, fixed); pinned receives the pinned rows of all
      ! ranks.  lbfgsb_qn_path_logdet: host only, logdet(j) = log det (B_FF + mu(j) I) where info(j) = 0 (1: theta +
      ! mu <= 0 or not finite, 2: not positive definite).  lbfgsb_qn_path_solve: out + (j-1)*ldo = (B_FF + mu(j) I)^-1
      ! v_F for k <= 64 shifts, norm2(j) = ||x_j||^2 and vx(j) = v'x_j; out may be c_null_ptr (the scalars alone).
      ! lbfgsb_qn_path_trust: step = -(B_FF + mu I)^-1 g_F with ||step|| <= delta; res = (mu, ||step||, the predicted
      ! decrease, on_boundary 0 / 1); rtol = 0 and max_it = 0 select 1e-10 and 100; step may be c_null_ptr.  After a
      ! return that stores a pair the last three return LBFGSB_E_STATE until lbfgsb_qn_path_set is called again.
      subroutine lbfgsb_qn_path_set(ctx, status, code_mask, pinned, rc)
      type(c_ptr),intent(in) :: ctx, status
      integer,intent(in) :: code_mask
      integer(c_int64_t),intent(out) :: pinned
      integer,intent(out) :: rc
      pinned = 0
      rc = lbfgsb_hip_qn_path_set(ctx, status, int(code_mask, c_int), pinned)
      end subroutine lbfgsb_qn_path_set

      subroutine lbfgsb_qn_path_logdet(ctx, k, mu, logdet, info, rc)
      type(c_ptr),intent(in) :: ctx
      integer,intent(in) :: k
      real(c_double),intent(in) :: mu(k)
      real(c_double),intent(out) :: logdet(k)
      integer(c_int32_t),intent(out) :: info(k)
      integer,intent(out) :: rc
      real(c_double) :: mus(k)
      mus = mu
      logdet = 0.0_c_double
      info = 0
      rc = lbfgsb_hip_qn_path_logdet(ctx, int(k, c_int64_t), mus, logdet, info)
      end subroutine lbfgsb_qn_path_logdet

      subroutine lbfgsb_qn_path_solve(ctx, v, k, mu, out, ldo, norm2, vx, rc)
      type(c_ptr),intent(in) :: ctx, v, out
      integer,intent(in) :: k, ldo
      real(c_double),intent(in) :: mu(k)
      real(c_double),intent(out) :: norm2(k), vx(k)
      integer,intent(out) :: rc
      real(c_double) :: mus(k)
      mus = mu
      norm2 = 0.0_c_double
      vx = 0.0_c_double
      rc = lbfgsb_hip_qn_path_solve(ctx, v, int(k, c_int64_t), mus, out, int(ldo, c_int64_t), norm2, vx)
      end subroutine lbfgsb_qn_path_solve

      subroutine lbfgsb_qn_path_trust(ctx, g, delta, rtol, max_it, step, res, iters, rc)
      type(c_ptr),intent(in) :: ctx, g, step
      real(c_double),intent(in) :: delta, rtol
      integer,intent(in) :: max_it
      real(c_double),intent(out) :: res(4)
      integer,intent(out) :: iters, rc
      integer(c_int32_t) :: it
      it = 0
      res = 0.0_c_double
      rc = lbfgsb_hip_qn_path_trust(ctx, g, delta, rtol, int(max_it, c_int), step, res, it)
      iters = int(it)
      end subroutine lbfgsb_qn_path_trust

      ! Square roots, draws and log-densities of the model plus a diagonal (include/lbfgsb_hip.h, "Square roots, draws
      ! and log-densities of the model plus a diagonal"): N(mean, scale^2 Sigma), Sigma = (B + mu I + D)^-1 on the free
      ! rows, after lbfgsb_qn_shift_set and under its staleness rule.  lbfgsb_qn_shift_sqrt: out_j = L v_j with L L' =
      ! Sigma, laid out as lbfgsb_qn_shift_solve's.  lbfgsb_qn_shift_draw: out_j = mean + scale L z_(first + j), j < k,
      ! z as lbfgsb_qn_draw's (mean may be c_null_ptr); a pinned row is its mean.  lbfgsb_qn_shift_draw_logpdf: the same
      ! draws and logp(j) = their log-densities.  lbfgsb_qn_shift_quad: q(j) = (v_j - center)'(B + mu I + D)(v_j -
      ! center) on the free rows.  lbfgsb_qn_shift_logpdf: logp(j) = log N(x_j; mean, scale^2 Sigma).  q and logp are
      ! host arrays, complete over the rows of all ranks; scale /= 0.
      subroutine lbfgsb_qn_shift_sqrt(ctx, k, v, ldv, out, ldo, rc)
      type(c_ptr),intent(in) :: ctx, v, out
      integer,intent(in) :: k, ldv, ldo
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_sqrt(ctx, int(k, c_int64_t), v, int(ldv, c_int64_t), out, int(ldo, c_int64_t))
      end subroutine lbfgsb_qn_shift_sqrt

      subroutine lbfgsb_qn_shift_draw(ctx, k, seed, first, mean, scale, out, ldo, rc)
      type(c_ptr),intent(in) :: ctx, mean, out
      integer,intent(in) :: k, first, ldo
      integer(c_int64_t),intent(in) :: seed
      real(c_double),intent(in) :: scale
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_draw(ctx, int(k, c_int64_t), seed, int(first, c_int64_t), mean, scale, out, &
                                    int(ldo, c_int64_t))
      end subroutine lbfgsb_qn_shift_draw

      subroutine lbfgsb_qn_shift_draw_logpdf(ctx, k, seed, first, mean, scale, out, ldo, logp, rc)
      type(c_ptr),intent(in) :: ctx, mean, out
      integer,intent(in) :: k, first, ldo
      integer(c_int64_t),intent(in) :: seed
      real(c_double),intent(in) :: scale
      real(c_double),intent(out) :: logp(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_draw_logpdf(ctx, int(k, c_int64_t), seed, int(first, c_int64_t), mean, scale, out, &
                                           int(ldo, c_int64_t), logp)
      end subroutine lbfgsb_qn_shift_draw_logpdf

      subroutine lbfgsb_qn_shift_quad(ctx, k, v, ldv, center, q, rc)
      type(c_ptr),intent(in) :: ctx, v, center
      integer,intent(in) :: k, ldv
      real(c_double),intent(out) :: q(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_quad(ctx, int(k, c_int64_t), v, int(ldv, c_int64_t), center, q)
      end subroutine lbfgsb_qn_shift_quad

      subroutine lbfgsb_qn_shift_logpdf(ctx, k, x, ldx, mean, scale, logp, rc)
      type(c_ptr),intent(in) :: ctx, x, mean
      integer,intent(in) :: k, ldx
      real(c_double),intent(in) :: scale
      real(c_double),intent(out) :: logp(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_logpdf(ctx, int(k, c_int64_t), x, int(ldx, c_int64_t), mean, scale, logp)
      end subroutine lbfgsb_qn_shift_logpdf

      ! Square roots, log-determinants and draws of the model (include/lbfgsb_hip.h, same block).  lbfgsb_qn_apply
      ! takes LBFGSB_QN_B_SQRT / LBFGSB_QN_H_SQRT for out_j = A^(1/2) v_j.  lbfgsb_qn_logdet: logdet = log det A over
      ! the rows of all ranks (mode LBFGSB_QN_B or LBFGSB_QN_H).  lbfgsb_qn_draw: out_j = mean + scale A^(1/2)
      ! z_(first + j), j < k, result j at out + j*ldo (device buffers of the context's real kind; mean may be
      ! c_null_ptr); z is generated on the device from seed (an integer(c_int64_t) holding the 64-bit pattern), the
      ! global row and the sample index alone.  At most 64 stored pairs.
      subroutine lbfgsb_qn_logdet(ctx, mode, logdet, rc)
      type(c_ptr),intent(in) :: ctx
      integer,intent(in) :: mode
      real(c_double),intent(out) :: logdet
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_logdet(ctx, int(mode, c_int), logdet)
      end subroutine lbfgsb_qn_logdet

      subroutine lbfgsb_qn_draw(ctx, mode, k, seed, first, mean, scale, out, ldo, rc)
      type(c_ptr),intent(in) :: ctx, mean, out
      integer,intent(in) :: mode, k, first, ldo
      integer(c_int64_t),intent(in) :: seed
      real(c_double),intent(in) :: scale
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_draw(ctx, int(mode, c_int), int(k, c_int64_t), seed, int(first, c_int64_t), mean, scale, &
                              out, int(ldo, c_int64_t))
      end subroutine lbfgsb_qn_draw

      ! Quadratic forms and Gaussian log-densities of the model (include/lbfgsb_hip.h, same block); every result is
      ! a host real(c_double) per vector, complete over the rows of all ranks.  lbfgsb_qn_quad: q(j) = (v_j - center)'
      ! A (v_j - center), mode LBFGSB_QN_B or LBFGSB_QN_H, center may be c_null_ptr.  lbfgsb_qn_logpdf: logp(j) = log
      ! N(x_j; mean, scale^2 A), mode naming the covariance A.  lbfgsb_qn_draw_logpdf: lbfgsb_qn_draw (the same
      ! draws bit for bit) and logp(j) = the log-density of draw j.  The last two: at most 64 stored pairs, scale /= 0.
      subroutine lbfgsb_qn_quad(ctx, mode, k, v, ldv, center, q, rc)
      type(c_ptr),intent(in) :: ctx, v, center
      integer,intent(in) :: mode, k, ldv
      real(c_double),intent(out) :: q(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_quad(ctx, int(mode, c_int), int(k, c_int64_t), v, int(ldv, c_int64_t), center, q)
      end subroutine lbfgsb_qn_quad

      ! g(a, b) = (v_a - center)' A (v_b - center), a, b <= k <= 64, a host array of leading dimension ldg >= k:
      ! both triangles, symmetric bit for bit; its diagonal is lbfgsb_qn_quad's (include/lbfgsb_hip.h, "Gram matrices")
      subroutine lbfgsb_qn_gram(ctx, mode, k, v, ldv, center, g, ldg, rc)
      type(c_ptr),intent(in) :: ctx, v, center
      integer,intent(in) :: mode, k, ldv, ldg
      real(c_double),intent(inout) :: g(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_gram(ctx, int(mode, c_int), int(k, c_int64_t), v, int(ldv, c_int64_t), center, g, &
                              int(ldg, c_int64_t))
      end subroutine lbfgsb_qn_gram

      ! Eigenvalues and eigenvectors of the model (include/lbfgsb_hip.h, "Eigenvalues and eigenvectors"): A = bulk I +
      ! U diag(lambda - bulk) U' with orthonormal U.  lbfgsb_qn_eig: bulk = theta (B) or 1 / theta (H), r the number
      ! of eigenvalues off it, lambda(1 : min(r, cap)) those in ascending order (a host array of at least cap >= 1
      ! entries; call with cap = 1 to learn r, at most 128).  lbfgsb_qn_eigvec: vector j = 1 .. k at out + (j - 1) ldo
      ! is the unit eigenvector of eigenvalue number which(j), 1-BASED into that list (repeats allowed), k <= 128.
      subroutine lbfgsb_qn_eig(ctx, mode, cap, r, bulk, lambda, rc)
      type(c_ptr),intent(in) :: ctx
      integer,intent(in) :: mode, cap
      integer,intent(out) :: r
      real(c_double),intent(out) :: bulk
      real(c_double),intent(inout) :: lambda(*)
      integer,intent(out) :: rc
      integer(c_int32_t) :: r32
      r32 = 0
      rc = lbfgsb_hip_qn_eig(ctx, int(mode, c_int), int(cap, c_int32_t), r32, bulk, lambda)
      r = int(r32)
      end subroutine lbfgsb_qn_eig

      subroutine lbfgsb_qn_eigvec(ctx, mode, k, which, out, ldo, rc)
      type(c_ptr),intent(in) :: ctx, out
      integer,intent(in) :: mode, k, ldo
      integer,intent(in) :: which(*)
      integer,intent(out) :: rc
      integer(c_int32_t) :: w0(128)
      integer :: j
      do j = 1, min(max(k, 0), 128)
         w0(j) = int(which(j) - 1, c_int32_t)
      end do
      rc = lbfgsb_hip_qn_eigvec(ctx, int(mode, c_int), int(k, c_int64_t), w0, out, int(ldo, c_int64_t))
      end subroutine lbfgsb_qn_eigvec

      subroutine lbfgsb_qn_logpdf(ctx, mode, k, x, ldx, mean, scale, logp, rc)
      type(c_ptr),intent(in) :: ctx, x, mean
      integer,intent(in) :: mode, k, ldx
      real(c_double),intent(in) :: scale
      real(c_double),intent(out) :: logp(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_logpdf(ctx, int(mode, c_int), int(k, c_int64_t), x, int(ldx, c_int64_t), mean, scale, logp)
      end subroutine lbfgsb_qn_logpdf

      subroutine lbfgsb_qn_draw_logpdf(ctx, mode, k, seed, first, mean, scale, out, ldo, logp, rc)
      type(c_ptr),intent(in) :: ctx, mean, out
      integer,intent(in) :: mode, k, first, ldo
      integer(c_int64_t),intent(in) :: seed
      real(c_double),intent(in) :: scale
      real(c_double),intent(out) :: logp(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_draw_logpdf(ctx, int(mode, c_int), int(k, c_int64_t), seed, int(first, c_int64_t), mean, &
                                     scale, out, int(ldo, c_int64_t), logp)
      end subroutine lbfgsb_qn_draw_logpdf

      ! Entries at index lists (include/lbfgsb_hip.h, "Entries at index lists").  idx, ia, ib are HOST arrays of GLOBAL
      ! 0-BASED int64 rows, as lbfgsb_kkt_list produces them (copied to the host); lists may be unsorted and repeat.
      ! lbfgsb_qn_rows: rows(j + (c - 1) ldr), j = 1 .. k, is entry idx(j) of logical column c of [S, Y] (c <= col: S,
      ! oldest pair first, then Y); k <= LBFGSB_QN_IDX_MAXK.  lbfgsb_qn_block: a(i + (j - 1) lda) = A(ia(i), ib(j)), A = B
      ! or H by mode; kb = 0 means ib = ia (ib is not read): the block is then symmetric bit for bit -- with
      ! LBFGSB_QN_H the marginal covariance of those parameters.  lbfgsb_qn_cols: column idx(j) of A at out + (j - 1)
      ! ldo (device memory, n reals each), k <= 128.  lbfgsb_qn_shift_block / _cols: the same for (B + mu I + diag(d))^-1
      ! of the shift in force (lbfgsb_qn_shift_set); pinned rows and columns are exactly +0.
      subroutine lbfgsb_qn_rows(ctx, k, idx, rows, ldr, rc)
      type(c_ptr),intent(in) :: ctx
      integer,intent(in) :: k, ldr
      integer(c_int64_t),intent(in) :: idx(*)
      real(c_double),intent(inout) :: rows(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_rows(ctx, int(k, c_int64_t), idx, rows, int(ldr, c_int64_t))
      end subroutine lbfgsb_qn_rows

      subroutine lbfgsb_qn_block(ctx, mode, ka, ia, kb, ib, a, lda, rc)
      type(c_ptr),intent(in) :: ctx
      integer,intent(in) :: mode, ka, kb, lda
      integer(c_int64_t),intent(in) :: ia(*)
      integer(c_int64_t),intent(in),target :: ib(*)
      real(c_double),intent(inout) :: a(*)
      integer,intent(out) :: rc
      type(c_ptr) :: pb
      pb = c_null_ptr
      if (kb > 0) pb = c_loc(ib)
      rc = lbfgsb_hip_qn_block(ctx, int(mode, c_int), int(ka, c_int64_t), ia, int(kb, c_int64_t), pb, a, &
                               int(lda, c_int64_t))
      end subroutine lbfgsb_qn_block

      subroutine lbfgsb_qn_cols(ctx, mode, k, idx, out, ldo, rc)
      type(c_ptr),intent(in) :: ctx, out
      integer,intent(in) :: mode, k, ldo
      integer(c_int64_t),intent(in) :: idx(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_cols(ctx, int(mode, c_int), int(k, c_int64_t), idx, out, int(ldo, c_int64_t))
      end subroutine lbfgsb_qn_cols

      subroutine lbfgsb_qn_shift_block(ctx, ka, ia, kb, ib, a, lda, rc)
      type(c_ptr),intent(in) :: ctx
      integer,intent(in) :: ka, kb, lda
      integer(c_int64_t),intent(in) :: ia(*)
      integer(c_int64_t),intent(in),target :: ib(*)
      real(c_double),intent(inout) :: a(*)
      integer,intent(out) :: rc
      type(c_ptr) :: pb
      pb = c_null_ptr
      if (kb > 0) pb = c_loc(ib)
      rc = lbfgsb_hip_qn_shift_block(ctx, int(ka, c_int64_t), ia, int(kb, c_int64_t), pb, a, int(lda, c_int64_t))
      end subroutine lbfgsb_qn_shift_block

      subroutine lbfgsb_qn_shift_cols(ctx, k, idx, out, ldo, rc)
      type(c_ptr),intent(in) :: ctx, out
      integer,intent(in) :: k, ldo
      integer(c_int64_t),intent(in) :: idx(*)
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_shift_cols(ctx, int(k, c_int64_t), idx, out, int(ldo, c_int64_t))
      end subroutine lbfgsb_qn_shift_cols

      ! Pairs in and out (include/lbfgsb_hip.h, "Pairs in and out: a curvature model of the caller's own").  s, y are
      ! DEVICE memory of the context's real kind: pair j (oldest first) at s + (j - 1) lds, y + (j - 1) ldy, n rows each.
      ! lbfgsb_qn_pairs_get: col = the stored pairs, theta; cap = 0 (s, y = c_null_ptr) counts only.  lbfgsb_qn_pairs_set:
      ! the context keeps the k <= m pairs as a model of the caller's own (it needs no run and ends the one it holds);
      ! theta = 0: y'y / s'y of the newest pair.  lbfgsb_qn_pairs_push: one more pair into such a model as matupd stores
      ! it; stored = 1, 0 (s'y not safely positive: nothing changed) or -1 (the model was reset to the empty one).
      subroutine lbfgsb_qn_pairs_get(ctx, cap, col, theta, s, lds, y, ldy, rc)
      type(c_ptr),intent(in) :: ctx, s, y
      integer,intent(in) :: cap, lds, ldy
      integer,intent(out) :: col, rc
      real(c_double),intent(out) :: theta
      integer(c_int32_t) :: c
      c = 0_c_int32_t
      theta = 0.0_c_double
      rc = lbfgsb_hip_qn_pairs_get(ctx, int(cap, c_int32_t), c, theta, s, int(lds, c_int64_t), y, int(ldy, c_int64_t))
      col = int(c)
      end subroutine lbfgsb_qn_pairs_get

      subroutine lbfgsb_qn_pairs_set(ctx, k, s, lds, y, ldy, theta, rc)
      type(c_ptr),intent(in) :: ctx, s, y
      integer,intent(in) :: k, lds, ldy
      real(c_double),intent(in) :: theta
      integer,intent(out) :: rc
      rc = lbfgsb_hip_qn_pairs_set(ctx, int(k, c_int32_t), s, int(lds, c_int64_t), y, int(ldy, c_int64_t), theta)
      end subroutine lbfgsb_qn_pairs_set

      subroutine lbfgsb_qn_pairs_push(ctx, s, y, theta, stored, rc)
      type(c_ptr),intent(in) :: ctx, s, y
      real(c_double),intent(in) :: theta
      integer,intent(out) :: stored, rc
      integer(c_int32_t) :: st
      st = 0_c_int32_t
      rc = lbfgsb_hip_qn_pairs_push(ctx, s, y, theta, st)
      stored = int(st)
      end subroutine lbfgsb_qn_pairs_push

      ! The active set, the multipliers and the projected gradient (include/lbfgsb_hip.h, "The active set, the bound
      ! multipliers and the projected gradient as device data"): one pass over the device arrays x, l, u, nbd, g of
      ! the context's real kind (nbd: int32).  pg, mult (reals) and status (one byte per row, iwhere's codes -1 .. 3)
      ! are device buffers or c_null_ptr (that output is then left out).  cnt(LBFGSB_KKT_N_*) and val(LBFGSB_KKT_*)
      ! are host arrays, complete over all ranks.  rc as the C entry returns it.
      subroutine lbfgsb_kkt(ctx, x, l, u, nbd, g, tol, pg, mult, status, cnt, val, rc)
      type(c_ptr),intent(in) :: ctx, x, l, u, nbd, g, pg, mult, status
      real(c_double),intent(in) :: tol
      integer(c_int64_t),intent(out) :: cnt(LBFGSB_KKT_NCNT)
      real(c_double),intent(out) :: val(LBFGSB_KKT_NVAL)
      integer,intent(out) :: rc
      cnt = 0_c_int64_t
      val = 0.0_c_double
      rc = lbfgsb_hip_kkt(ctx, x, l, u, nbd, g, tol, pg, mult, status, cnt, val)
      end subroutine lbfgsb_kkt

      ! The rows whose status byte is selected by code_mask (bit code + 1; e.g. 12 = at a lower or an upper bound),
      ! ascending, as GLOBAL 0-based int64 indices (row0 + i) into the device buffer idx: at most cap of them, count
      ! receives this rank's full count.  idx = c_null_ptr with cap = 0 is the counting call.
      subroutine lbfgsb_kkt_list(ctx, status, code_mask, idx, cap, count, rc)
      type(c_ptr),intent(in) :: ctx, status, idx
      integer,intent(in) :: code_mask
      integer(c_int64_t),intent(in) :: cap
      integer(c_int64_t),intent(out) :: count
      integer,intent(out) :: rc
      count = 0_c_int64_t
      rc = lbfgsb_hip_kkt_list(ctx, status, int(code_mask, c_int), idx, cap, count)
      end subroutine lbfgsb_kkt_list

      function lbfgsb_error_message() result(msg)
      character(len=:),allocatable :: msg
      type(c_ptr) :: p
      character(kind=c_char),pointer :: cs(:)
      integer :: k, i
      p = lbfgsb_hip_last_error()
      msg = ''
      if (.not. c_associated(p)) return
      k = int(c_strlen(p))
      if (k <= 0) return
      call c_f_pointer(p, cs, [k])
      allocate (character(len=k) :: msg)
      do i = 1, k
         msg(i:i) = cs(i)
      end do
      end function lbfgsb_error_message

      subroutine lbfgsb_release(Isave)
      integer :: Isave(44)
      integer(c_int32_t) :: rc
      rc = lbfgsb_hip_release_host_ik(Isave, int(ibytes, c_int32_t))
      end subroutine lbfgsb_release

      end module lbfgsb_module
