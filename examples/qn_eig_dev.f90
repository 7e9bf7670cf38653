!  qn_eig_dev -- qn_gram_dev's loop (the reference's test/driver2.f90:66-195 on device buffers, the library's
!  built-in separable bounded quadratic, classic entry setulb_dev), then the spectrum of H = B^-1 at the last iterate
!  (lbfgsb_qn_eig): the bulk eigenvalue 1 / theta and the r eigenvalues off it, ascending, and for the eigenvector u
!  of the largest one (lbfgsb_qn_eigvec) the residual |H u - lambda u| with H u from lbfgsb_qn_apply, and |u|.
!
!     qn_eig_dev [n [m [iterations]]]      defaults 100000, 5, 12
!
!  Output: one "Iterate" line per iterate, then
!     QNEIG col = <stored pairs> r = <eigenvalues off the bulk value>
!     QNEIG bulk <1 / theta>
!     QNEIG lambda <index> <eigenvalue>                  (r lines)
!     QNEIG top <lambda> <|H u - lambda u|> <|u|>
      program qn_eig_dev

      use lbfgsb_module, wp => lbfgsp_wp
      use iso_c_binding
      use iso_fortran_env, only: output_unit

      implicit none

      interface
         function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr) :: ptr
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMalloc
         function hipFree(ptr) bind(C, name='hipFree') result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: ptr
            integer(c_int) :: rc
         end function hipFree
         function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: nbytes
            integer(c_int), value :: kind
            integer(c_int) :: rc
         end function hipMemcpy
         function hipMemset(dst, val, nbytes) bind(C, name='hipMemset') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst
            integer(c_int), value :: val
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMemset
      end interface
      integer(c_int), parameter :: H2D = 1, D2H = 2

      integer               :: n, m, maxit, rc, i
      real(wp), parameter   :: factr = 0.0_wp, pgtol = 0.0_wp
      character(len=60)     :: task, csave
      character(len=32)     :: arg
      logical               :: lsave(4)
      integer               :: isave(44)
      real(wp)              :: f, dsave(29)
      real(c_double)        :: bulk, lambda(128), res, unorm
      type(c_ptr)           :: ctx, dx, dg, dl, du, dnbd, du1, dhu
      real(wp), allocatable, target :: hu(:)
      integer               :: a, r, top(1)
      real(wp), allocatable, target :: hbuf(:)
      integer(c_int32_t), allocatable, target :: hnbd(:)
      integer(c_size_t)     :: vbytes

      n = 100000; m = 5; maxit = 12
      if (command_argument_count() >= 1) then
         call get_command_argument(1, arg); read (arg, *) n
      end if
      if (command_argument_count() >= 2) then
         call get_command_argument(2, arg); read (arg, *) m
      end if
      if (command_argument_count() >= 3) then
         call get_command_argument(3, arg); read (arg, *) maxit
      end if

      vbytes = int(n, c_size_t)*int(storage_size(1.0_wp)/8, c_size_t)
      call chk(hipMalloc(dx, vbytes), 'hipMalloc x')
      call chk(hipMalloc(dg, vbytes), 'hipMalloc g')
      call chk(hipMalloc(dl, vbytes), 'hipMalloc l')
      call chk(hipMalloc(du, vbytes), 'hipMalloc u')
      call chk(hipMalloc(du1, vbytes), 'hipMalloc u')
      call chk(hipMalloc(dhu, vbytes), 'hipMalloc H u')
      call chk(hipMalloc(dnbd, int(n, c_size_t)*4_c_size_t), 'hipMalloc nbd')
      call chk(hipMemset(dx, 0_c_int, vbytes), 'hipMemset x')             ! x0 = 0
      call chk(hipMemset(dg, 0_c_int, vbytes), 'hipMemset g')
      allocate (hbuf(n))
      hbuf = -1.0_wp                                                       ! l = -1
      call chk(hipMemcpy(dl, c_loc(hbuf), vbytes, H2D), 'hipMemcpy l')
      hbuf = 1.0_wp                                                        ! u = +1
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy u')
      allocate (hnbd(n))
      do i = 1, n
         hnbd(i) = int(mod(i, 4), c_int32_t)                               ! all four bound types
      end do
      call chk(hipMemcpy(dnbd, c_loc(hnbd), int(n, c_size_t)*4_c_size_t, H2D), 'hipMemcpy nbd')
      deallocate (hnbd)

      call lbfgsb_create(ctx, n, m, 0, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_create failed: ', lbfgsb_error_message()
         error stop 1
      end if

      task = 'START'
      f = 0.0_wp
      do while (task(1:2) == 'FG' .or. task == 'NEW_X' .or. task == 'START')
         call setulb_dev(ctx, dx, dl, du, dnbd, f, dg, factr, pgtol, task, -1, csave, lsave, isave, dsave, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' setulb_dev failed: ', lbfgsb_error_message()
            error stop 1
         end if
         if (task(1:2) == 'FG') then
            call lbfgsb_objective(ctx, 0, dx, dg, rc, f)
            if (rc /= 0) error stop 2
         else if (task(1:5) == 'NEW_X') then
            write (output_unit, '(2(a,i5,4x),a,1p,d12.5,4x,a,1p,d12.5)') 'Iterate', isave(30), 'nfg =', isave(34), &
               'f =', f, '|proj g| =', dsave(13)
            if (isave(30) >= maxit) exit                                   ! the model of this NEW_X return
         end if
      end do

      ! the spectrum of H, the eigenvector of its largest eigenvalue and the residual of that pair
      call lbfgsb_qn_eig(ctx, LBFGSB_QN_H, 128, r, bulk, lambda, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_eig failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,i4,a,i4)') 'QNEIG col =', isave(28), ' r =', r
      write (output_unit, '(a,es25.16e3)') 'QNEIG bulk', bulk
      do a = 1, r
         write (output_unit, '(a,i4,es25.16e3)') 'QNEIG lambda', a, lambda(a)
      end do
      if (r >= 1) then
         top(1) = r
         call lbfgsb_qn_eigvec(ctx, LBFGSB_QN_H, 1, top, du1, n, rc)
         if (rc == 0) call lbfgsb_qn_apply(ctx, LBFGSB_QN_H, 1, du1, n, dhu, n, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' lbfgsb_qn_eigvec / lbfgsb_qn_apply failed: ', lbfgsb_error_message()
            error stop 1
         end if
         allocate (hu(n))
         call chk(hipMemcpy(c_loc(hu), du1, vbytes, D2H), 'hipMemcpy u')
         call chk(hipMemcpy(c_loc(hbuf), dhu, vbytes, D2H), 'hipMemcpy H u')
         res = 0.0_c_double; unorm = 0.0_c_double
         do i = 1, n
            res = res + (real(hbuf(i), c_double) - lambda(r)*real(hu(i), c_double))**2
            unorm = unorm + real(hu(i), c_double)**2
         end do
         write (output_unit, '(a,3es25.16e3)') 'QNEIG top', lambda(r), sqrt(res), sqrt(unorm)
         deallocate (hu)
      end if

      task = 'STOP: QN_EIG_DEV'
      call lbfgsb_destroy(ctx)
      rc = hipFree(dx); rc = hipFree(dg); rc = hipFree(dl); rc = hipFree(du)
      rc = hipFree(du1); rc = hipFree(dnbd); rc = hipFree(dhu)

      contains

      subroutine chk(code, what)
      integer(c_int), intent(in) :: code
      character(len=*), intent(in) :: what
      if (code /= 0) then
         write (output_unit, '(3a,i0)') ' ', what, ' failed, hipError ', code
         error stop 3
      end if
      end subroutine chk

      end program qn_eig_dev
